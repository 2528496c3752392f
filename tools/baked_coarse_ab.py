"""The baked coarse pass on the bench frame (800x800, 8x256, 64+128, the benchmark's networks): arms alternating on one box, three
repetitions each:

  none        no grid: the ordinary frame (fused kernel, work queue and tail path as the context picks them)
  baked 128   the coarse network's density baked at 128^3 over the scene box
  baked 256   ... at 256^3

Per arm: kernel ms, the producer's ms, executed / full ray evaluations, and against the unbaked frame max |d rgb|, the share of
rays above 1e-4 and the PSNR.  Prints one line per (arm, repetition) and a summary of medians with their spread; DESIGN.md
section 5.7 quotes it.  Read the time against the 23.5 % of the frame's MFMAs the coarse pass holds, and against the 2 - 3.5 %
the work queue and the tail path gave, which the baked main stage (the sharing consumer, not queued) does not have.
Usage on the GPU box: python tools/baked_coarse_ab.py [H W]."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nwe_amd
from nwe_amd import synthetic

H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (800, 800)
pose = np.array([[0.8660254, 0, 0.5, 0], [-0.5, 0, 0.8660254, -0.76157], [0, -1, 0, 0.5], [0, 0, 0, 1]], np.float32)
fx, fy, cx, cy = nwe_amd.pinhole_intrinsics(H, W)
LO, HI = (-16.0, -16.0, -16.0), (16.0, 16.0, 16.0)      # every sample of the frame (depth 0.1 .. 10 from (0, -0.76, 0.5))


def frame(r):
    return r.render(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "depth", "acc"))


def baked(res):
    def enter(r):
        t0 = time.perf_counter()
        r.bake_coarse_grid(LO, HI, res)
        print(f"bake {res}^3: {1e3 * (time.perf_counter() - t0):.1f} ms", flush=True)
    return enter


def main():
    r = nwe_amd.Renderer(0)
    r.set_network(0, synthetic.make_state_dict(1000, 8, 256))
    r.set_network(1, synthetic.make_state_dict(1001, 8, 256))
    r.set_sampling(64, 128)
    arms = (("none", lambda r: r.clear_coarse_grid()), ("baked 128", baked(128)), ("baked 256", baked(256)))
    ms, prod, ran, rgb = {a: [] for a, _ in arms}, {a: [] for a, _ in arms}, {}, {}
    full = 0
    for rep in range(3):
        for label, enter in arms:
            enter(r)
            for i in range(3):      # one launch to warm up, two timed
                out = frame(r)
                if i > 0:
                    ms[label].append(r.last_kernel_ms())
                    c = r.last_coarse_launch()
                    prod[label].append(c[0] if c else 0.0)
            ran[label], full = r.last_ray_evaluations()
            rgb[label] = out["rgb"]
            print(f"{label} rep {rep}: kernel {ms[label][-2]:.2f} / {ms[label][-1]:.2f} ms, producer {prod[label][-2]:.3f} / {prod[label][-1]:.3f} ms, "
                  f"evaluations {ran[label]} of {full} ({100.0 * ran[label] / full:.1f} %)", flush=True)
    base = statistics.median(ms["none"])
    print(f"== none: median {base:.2f} ms ({min(ms['none']):.2f} - {max(ms['none']):.2f})", flush=True)
    for label, _ in arms[1:]:
        t = statistics.median(ms[label])
        d = (rgb[label] - rgb["none"]).abs()
        mse = float((d.double() ** 2).mean())
        psnr = "inf" if mse == 0 else f"{-10.0 * np.log10(mse):.1f}"
        print(f"== {label}: median {t:.2f} ms ({min(ms[label]):.2f} - {max(ms[label]):.2f}) vs {base:.2f} ms ({100 * (1.0 - t / base):+.1f} % time saved), "
              f"producer {statistics.median(prod[label]):.3f} ms, {100 * (1.0 - ran[label] / full):.1f} % of the evaluations saved; "
              f"max |d rgb| {float(d.max()):.2e}, rays above 1e-4 {100 * float((d.max(-1).values > 1e-4).float().mean()):.2f} %, PSNR {psnr} dB", flush=True)
    r.close()


if __name__ == "__main__":
    main()
