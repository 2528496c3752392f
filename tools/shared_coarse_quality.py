"""What the shared coarse pass (include/nwe.h: nwe_set_shared_coarse) costs in quality, on the CPU oracle: 16 patches of 16x16
pixels on a 4x4 grid over the 800x800 frame of tests/early_termination.frame_rays pose 0 (4096 rays per scene), 8x256,
64+128.  Every ray's fine pass is evaluated at its representative's z_fine and compared with the ordinary frame: max / mean
|d rgb|, PSNR, max |d depth|, and the share of 8-bit values that change after to8b.  DESIGN.md section 5.2 quotes it;
tools/shared_coarse_ab.py measures the same over every ray of the frame on the GPU.  Usage: python tools/shared_coarse_quality.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nwe_amd
from oracle import nerf_oracle as O
from tests import early_termination as E
from tests import shared_coarse as SC

H = W = 800
P = 16                                               # patch edge: a multiple of every k, so blocks lie inside patches
corners = [(r0, c0) for r0 in (48, 272, 496, 720) for c0 in (32, 256, 480, 736)]
rays = E.frame_rays(H, W)[1].reshape(H, W, 11)
patch = torch.cat([rays[r0:r0 + P, c0:c0 + P].reshape(-1, 11) for r0, c0 in corners])
S = nwe_amd.synthetic
t = lambda sd: {k: torch.from_numpy(v) for k, v in sd.items()}
raw = lambda seed: S.make_state_dict(seed, 8, 256)
fog = lambda sd: S.dense_fog(sd, 0.5, 3.0)
scenes = (("bench", raw(1000), raw(1001)), ("posfog", fog(raw(1000)), fog(raw(1001))),
          ("thin+posfog", S.thin_fog(raw(1000)), fog(raw(1001))), ("thin", S.thin_fog(raw(1000)), S.thin_fog(raw(1001))))
cfg = O.RenderConfig(64, 128)
for name, coarse, fine in scenes:
    ref = O.render_rays(patch, t(coarse), t(fine), cfg, keep=("rgb_fine", "depth_fine", "z_fine"))
    for k in (2, 4):
        # a patch is a P x P image of its own for the block arithmetic: its corner is a multiple of k
        rep = np.concatenate([i * P * P + SC.rep_index(P, P, k, 0, P, 1) for i in range(len(corners))])
        out = O.fine_pass_given_depths(patch, ref["z_fine"][torch.from_numpy(rep)], t(fine), cfg)
        d = (out["rgb_fine"] - ref["rgb_fine"]).abs()
        mse = float(((out["rgb_fine"] - ref["rgb_fine"]).double() ** 2).mean())
        changed = float((O.to8b(out["rgb_fine"].numpy()) != O.to8b(ref["rgb_fine"].numpy())).mean())
        print(f"{name} k {k} over {len(patch)} rays: max |d rgb| {float(d.max()):.2e}, mean {float(d.mean()):.2e}, PSNR "
              f"{-10.0 * np.log10(max(mse, 1e-30)):.1f} dB, max |d depth| {float((out['depth_fine'] - ref['depth_fine']).abs().max()):.2e}, "
              f"8-bit values changed {100 * changed:.2f} %", flush=True)
