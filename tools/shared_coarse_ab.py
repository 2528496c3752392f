"""The shared coarse pass on the C3 frame (800x800, 8x256, 64+128): kernel time, the producer's time and executed / full ray
evaluations for k in {1, 2, 4}, alternating on one box, three repetitions of two timed launches, medians; then what the rule
costs in quality against the ordinary frame of the same kernels, over every ray of the frame, on four scenes:

  bench       the benchmark's raw random networks (no surfaces, no coherence: the roughest case);
  posfog      a position-dependent fog (sigma 0.5, spread 3.0) in both networks;
  thin+posfog a thin-fog coarse network under that fine network;
  thin        thin fog in both.

Prints one line per (k, repetition), a summary with the time saved against the MFMAs saved (DESIGN.md section 5.2 quotes
it), and per scene and k: max / mean |d rgb|, PSNR, max |d depth| and the share of 8-bit values that change after to8b.
Usage on the GPU box: python tools/shared_coarse_ab.py [H W]."""
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nwe_amd
from nwe_amd import synthetic

KS = (1, 2, 4)
H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (800, 800)
pose = np.array([[0.8660254, 0, 0.5, 0], [-0.5, 0, 0.8660254, -0.76157], [0, -1, 0, 0.5], [0, 0, 0, 1]], np.float32)
fx, fy, cx, cy = nwe_amd.pinhole_intrinsics(H, W)
raw = lambda seed: synthetic.make_state_dict(seed, 8, 256)
# MFMAs per evaluation: density-only coarse 2880, fine 3120
MFMA_COARSE, MFMA_FINE = 2880, 3120


def renderer(coarse, fine):
    r = nwe_amd.Renderer(0)
    r.set_network(0, coarse)
    r.set_network(1, fine)
    r.set_sampling(64, 128)
    return r


def frame(r):
    return r.render(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "depth", "acc"))


r = renderer(raw(1000), raw(1001))
ms, coarse_ms, ran, reps = {k: [] for k in KS}, {k: [] for k in KS}, {}, {}
for rep in range(3):
    for k in KS:
        r.set_shared_coarse(k)
        for i in range(3):      # one launch to warm up, two timed
            frame(r)
            if i > 0:
                ms[k].append(r.last_kernel_ms())
                coarse_ms[k].append((r.last_coarse_launch() or (0.0, 0))[0])
        ran[k], full = r.last_ray_evaluations()
        reps[k] = (r.last_coarse_launch() or (0.0, 0))[1]
        print(f"bench k {k} rep {rep}: kernel {ms[k][-2]:.2f} / {ms[k][-1]:.2f} ms, producer {coarse_ms[k][-2]:.2f} / {coarse_ms[k][-1]:.2f} ms "
              f"over {reps[k]} rays, consumer parts {r.last_launch_parts()}, evaluations {ran[k]} of {full} ({100.0 * ran[k] / full:.1f} %)",
              flush=True)
base = statistics.median(ms[1])
n_rays = H * W
mfma_full = n_rays * (64 * MFMA_COARSE + 192 * MFMA_FINE)
for k in KS[1:]:
    t = statistics.median(ms[k])
    saved_t = 1.0 - t / base
    saved_m = (n_rays - reps[k]) * 64 * MFMA_COARSE / mfma_full
    print(f"== bench k {k}: median {t:.2f} ms (producer {statistics.median(coarse_ms[k]):.2f} ms) vs {base:.2f} ms at k 1: "
          f"{100 * saved_t:+.1f} % time saved for {100 * saved_m:.1f} % of the MFMAs saved (ratio {saved_t / saved_m:.2f}); "
          f"{100 * (1.0 - ran[k] / full):.1f} % of the evaluations saved", flush=True)
r.close()

fog = lambda sd: synthetic.dense_fog(sd, 0.5, 3.0)
scenes = (("bench", raw(1000), raw(1001)), ("posfog", fog(raw(1000)), fog(raw(1001))),
          ("thin+posfog", synthetic.thin_fog(raw(1000)), fog(raw(1001))), ("thin", synthetic.thin_fog(raw(1000)), synthetic.thin_fog(raw(1001))))
for name, coarse, fine in scenes:
    r = renderer(coarse, fine)
    plain = frame(r)
    plain8 = r.to8b(plain["rgb"])
    for k in KS[1:]:
        r.set_shared_coarse(k)
        out = frame(r)
        d = (out["rgb"] - plain["rgb"]).abs()
        mse = float(((out["rgb"] - plain["rgb"]).double() ** 2).mean())
        changed = float((r.to8b(out["rgb"]) != plain8).float().mean())
        print(f"== quality {name} k {k} over {n_rays} rays: max |d rgb| {float(d.max()):.2e}, mean {float(d.mean()):.2e}, "
              f"PSNR {-10.0 * math.log10(max(mse, 1e-30)):.1f} dB, max |d depth| {float((out['depth'] - plain['depth']).abs().max()):.2e}, "
              f"8-bit values changed {100 * changed:.2f} %", flush=True)
    r.close()
