#!/usr/bin/env python3
"""The bench frame's hollow (wave, sample) pairs, counted on the GPU: pairs of a wave's 32 rays and a fine sample at which no
ray of the wave has density (sigma_raw <= 0), by raw_fine of the full instantiation, which never takes the hollow path.  Counted
for packets of 32 consecutive pixels of a row and for packets of 8x4 pixel blocks (csrc/nwe_packet_blocks.h), with the
SQ_INSTS_MFMA per frame that follows from each: a hollow pair leaves out 186 of the 240 colour MFMAs of an 8x256 evaluation.

    python tools/hollow_count.py            -> one JSON line
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import nwe_amd  # noqa: E402
from nwe_amd.handler import pinhole_intrinsics  # noqa: E402

ROWS = 40                       # rows per call: 32 000 rays x 192 samples x 16 B of raw_fine = 98 MB
MFMA_ALL = 15_667_200_000       # per frame with every colour layer evaluated in the fine pass
MFMA_COLOUR = 186               # view tiles 1 .. NTV-1 and the rgb head of one 8x256 evaluation, three-pass: what a hollow wave leaves out


def main():
    H, W = bench.H, bench.W
    assert H % ROWS == 0 and ROWS % 4 == 0 and W % 32 == 0
    r = nwe_amd.Renderer(0)
    r.set_network(0, nwe_amd.synthetic.make_state_dict(1000, 8, 256))
    r.set_network(1, nwe_amd.synthetic.make_state_dict(1001, 8, 256))
    r.set_sampling(bench.NS, bench.NI)
    fx, fy, cx, cy = pinhole_intrinsics(H, W)   # the handler's, as bench.py renders the frame: near 0.1, far 10
    pose = bench.sweep_pose(0, 1)
    flt_max = float(np.finfo(np.float32).max)
    strips = blocks = pairs = samples = 0
    for r0 in range(0, H, ROWS):
        out = r.render(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, rows=(r0, r0 + ROWS),
                       outputs=("rgb", "raw_fine"))
        sigma = out["raw_fine"][..., 3]
        none = ((sigma <= 0) & (sigma >= -flt_max)).view(ROWS, W, -1)                   # [row, column, sample]
        S = none.shape[-1]
        strips += int(none.view(ROWS, W // 32, 32, S).all(dim=2).sum())
        blocks += int(none.view(ROWS // 4, 4, W // 8, 8, S).all(dim=3).all(dim=1).sum())
        pairs += ROWS * W // 32 * S
        samples += int(none.sum())
    r.close()
    print(json.dumps({"pairs": pairs, "samples_without_density": samples / (pairs * 32),
                      "hollow_pairs_strips": strips, "hollow_share_strips": strips / pairs,
                      "hollow_pairs_blocks": blocks, "hollow_share_blocks": blocks / pairs,
                      "mfma_all": MFMA_ALL, "mfma_left_out_per_hollow_pair": MFMA_COLOUR,
                      "mfma_predicted_strips": MFMA_ALL - MFMA_COLOUR * strips,
                      "mfma_predicted_blocks": MFMA_ALL - MFMA_COLOUR * blocks}))


if __name__ == "__main__":
    main()
