"""Early ray termination on the C3 frame (800x800, 8x256): kernel time and executed / full ray evaluations for
min_transmittance in {0, 1e-4, 1e-2}, alternating on one box, three repetitions each, on three scenes:

  bench    the benchmark's raw random networks, 64+128: nothing terminates, so this is the price of the vote;
  fog      dense fog (sigma 3, spread 0.01), 64+128: every ray stops in the fine pass;
  fog64+0  the same fog, 64 coarse samples only: the only pass is the terminated one.

Prints one line per (scene, eps, repetition) and a summary of medians with the time saved per evaluation saved
(DESIGN.md section 5.x quotes it).  Usage on the GPU box: python tools/early_termination_ab.py [H W]."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nwe_amd
from nwe_amd import synthetic

EPS = (0.0, 1e-4, 1e-2)
H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (800, 800)
pose = np.array([[0.8660254, 0, 0.5, 0], [-0.5, 0, 0.8660254, -0.76157], [0, -1, 0, 0.5], [0, 0, 0, 1]], np.float32)
fx, fy, cx, cy = nwe_amd.pinhole_intrinsics(H, W)
fog = lambda seed: synthetic.dense_fog(synthetic.make_state_dict(seed, 8, 256))
scenes = (("bench", synthetic.make_state_dict(1000, 8, 256), synthetic.make_state_dict(1001, 8, 256), 64, 128),
          ("fog", fog(1000), fog(1001), 64, 128),
          ("fog64+0", fog(1000), None, 64, 0))

for name, coarse, fine, ns, ni in scenes:
    r = nwe_amd.Renderer(0)
    r.set_network(0, coarse)
    if fine is not None:
        r.set_network(1, fine)
    r.set_sampling(ns, ni)
    ms, ran = {e: [] for e in EPS}, {}
    for rep in range(3):
        for eps in EPS:
            r.set_early_termination(eps)
            for i in range(3):      # one launch to warm up, two timed
                r.render(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "depth", "acc"))
                if i > 0:
                    ms[eps].append(r.last_kernel_ms())
            ran[eps], full = r.last_ray_evaluations()
            print(f"{name} eps {eps:g} rep {rep}: kernel {ms[eps][-2]:.2f} / {ms[eps][-1]:.2f} ms, evaluations {ran[eps]} of {full} "
                  f"({100.0 * ran[eps] / full:.1f} %)", flush=True)
    base = statistics.median(ms[0.0])
    for eps in EPS[1:]:
        t = statistics.median(ms[eps])
        saved_t, saved_e = 1.0 - t / base, 1.0 - ran[eps] / full
        ratio = f", time saved per evaluation saved {saved_t / saved_e:.2f}" if saved_e > 0 else ""
        print(f"== {name} eps {eps:g}: median {t:.2f} ms vs {base:.2f} ms at eps 0 ({100 * saved_t:+.1f} % time saved), "
              f"{100 * saved_e:.1f} % of the evaluations saved{ratio}", flush=True)
    r.close()
