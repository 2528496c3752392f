"""Separate passes on the C3 frame (800x800, 64+128, f16x3), alternating on one box, three repetitions of two timed launches,
medians (DESIGN.md section 5.3 quotes them):

  fused      8x256 / 8x256, the mode off: one launch;
  separate   8x256 / 8x256, the mode on: a coarse and a fine launch and the weight table between them (the frame must be the
             fused one bit for bit, which is checked);
  mixed      4x128 coarse + 8x256 fine, the mode on;
  mixed-f32  the same pair under f32, what that pair renders with when the mode is off.

Prints one line per (variant, repetition) and a summary: the medians, the coarse launch's share, and the time saved by the
small coarse network against the MFMAs it saves (per evaluation, from the packed tile counts: 1.5 MFMAs per 1-KiB tile, a
(hi, lo) pair of tiles per k-step and three products).
Usage on the GPU box: python tools/separate_passes_ab.py [H W]."""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nwe_amd
from nwe_amd import synthetic

H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (800, 800)
NS, NI = 64, 128
pose = np.array([[0.8660254, 0, 0.5, 0], [-0.5, 0, 0.8660254, -0.76157], [0, -1, 0, 0.5], [0, 0, 0, 1]], np.float32)
fx, fy, cx, cy = nwe_amd.pinhole_intrinsics(H, W)


def renderer(coarse, fine, on):
    r = nwe_amd.Renderer(0)
    r.set_network(0, synthetic.make_state_dict(1000, *coarse))
    r.set_network(1, synthetic.make_state_dict(1001, *fine))
    r.set_sampling(NS, NI)
    r.set_separate_passes(on)
    return r


def frame(r, precision):
    return r.render(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, precision=precision, outputs=("rgb", "depth", "acc"))


def mfmas(r, which, density_only):
    """MFMAs of one evaluation of network `which`; a density-only evaluation leaves out the view layer (W/2 rows over W + 32
    columns) and the rgb head (32 rows over W/2 columns): tiles of 32 rows, k-steps of 16, three products."""
    full = r.packed_stream(which).size // 1024 * 3 // 2
    width = r.shapes[which][1]
    return full - (3 * (width // 2 // 32) * ((width + 32) // 16) + 3 * (width // 2 // 16) if density_only else 0)


VARIANTS = {"fused": ((8, 256), (8, 256), False, "f16x3"), "separate": ((8, 256), (8, 256), True, "f16x3"),
            "mixed": ((4, 128), (8, 256), True, "f16x3"), "mixed-f32": ((4, 128), (8, 256), True, "f32")}
rs = {name: renderer(c, f, on) for name, (c, f, on, _) in VARIANTS.items()}
a, b = frame(rs["fused"], "f16x3"), frame(rs["separate"], "f16x3")
print("separate == fused, bit for bit:", all(torch.equal(a[k], b[k]) for k in ("rgb", "depth", "acc", "flags")), flush=True)
ms, coarse_ms = {n: [] for n in VARIANTS}, {n: [] for n in VARIANTS}
for rep in range(3):
    for name, (_, _, _, precision) in VARIANTS.items():
        r = rs[name]
        if precision == "f32" and rep > 0:                   # ~25x the time of the others: one repetition
            continue
        for i in range(3 if precision != "f32" else 2):      # one launch to warm up, two (f32: one) timed
            frame(r, precision)
            if i > 0:
                ms[name].append(r.last_kernel_ms())
                coarse_ms[name].append((r.last_coarse_launch() or (0.0, 0))[0])
        print(f"{name} rep {rep}: kernel {ms[name][-1]:.2f} ms, coarse launch {coarse_ms[name][-1]:.2f} ms, fine parts {r.last_launch_parts()}, "
              f"plan {r.debug_last_plan()}, evaluations {r.last_ray_evaluations()}", flush=True)
med = {n: statistics.median(v) for n, v in ms.items()}
for name in VARIANTS:
    print(f"== {name}: median {med[name]:.2f} ms (coarse launch {statistics.median(coarse_ms[name]):.2f} ms), min {min(ms[name]):.2f}, max {max(ms[name]):.2f}")
print(f"== separate vs fused: {100 * (med['separate'] / med['fused'] - 1):+.2f} %")
m_c8, m_f8 = mfmas(rs["fused"], 0, True), mfmas(rs["fused"], 1, False)
m_c4 = mfmas(rs["mixed"], 0, True)
full8, mixed = NS * m_c8 + (NS + NI) * m_f8, NS * m_c4 + (NS + NI) * m_f8
print(f"== MFMAs per evaluation: 8x256 density-only {m_c8}, 8x256 full {m_f8}, 4x128 density-only {m_c4}; per ray {full8} fused 8x256, "
      f"{mixed} mixed: {100 * (mixed / full8 - 1):+.1f} % predicted, {100 * (med['mixed'] / med['fused'] - 1):+.1f} % measured; "
      f"mixed f16x3 vs the same pair under f32: {med['mixed-f32'] / med['mixed']:.1f}x")
for r in rs.values():
    r.close()
