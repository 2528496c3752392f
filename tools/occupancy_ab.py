"""The occupancy grid on the C3 frame (800x800, 8x256, 64+128): kernel time and executed / full ray evaluations, arms alternating
on one box, three repetitions each:

  ask    the benchmark's raw random networks with an ALL-SET grid at 128^3 and 256^3 against no grid: the price of asking
         (the load, the vote and its barrier; the grid shares the L2 with the weight stream);
  built  the same networks with a grid built from them (resolution 128, probes 2, threshold 0, dilate 0 and 1): executed /
         full, ms, and against the plain frame max |d rgb|, the share of rays above 1e-4 and the PSNR;
  slab   a slab network (sigma_raw = relu(k x / 10 + b): exactly 0 below x0) with its exact grid: any time saved is free.

Prints one line per (scene, arm, repetition) and a summary of medians with the time saved per evaluation saved (DESIGN.md
section 5.6 quotes it).  Usage on the GPU box: python tools/occupancy_ab.py [H W]."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nwe_amd
from nwe_amd import synthetic

H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (800, 800)
pose = np.array([[0.8660254, 0, 0.5, 0], [-0.5, 0, 0.8660254, -0.76157], [0, -1, 0, 0.5], [0, 0, 0, 1]], np.float32)
fx, fy, cx, cy = nwe_amd.pinhole_intrinsics(H, W)
LO, HI = (-16.0, -16.0, -16.0), (16.0, 16.0, 16.0)      # every sample of the frame (depth 0.1 .. 10 from (0, -0.76, 0.5))
K, B = 8.0, -4.8                                         # the slab: x0 = -10 b / k = 6


def slab(seed):
    sd = synthetic.make_state_dict(seed, 8, 256)
    sd["_pts_linears.0.weight"][0] = 0.0
    sd["_pts_linears.0.weight"][0, 0] = K
    sd["_pts_linears.0.bias"][0] = B
    for i in range(1, 8):
        w = sd[f"_pts_linears.{i}.weight"]
        w[0] = 0.0
        w[0, 63 if w.shape[1] == 256 + 63 else 0] = 1.0
        sd[f"_pts_linears.{i}.bias"][0] = 0.0
    sd["_alpha_linear.weight"][:] = 0.0
    sd["_alpha_linear.weight"][0, 0] = 1.0
    sd["_alpha_linear.bias"][:] = 0.0
    return sd


def slab_bits(res):
    cell = (HI[0] - LO[0]) / res
    upper = LO[0] + (np.arange(res) + 1) * cell
    return np.ascontiguousarray(np.broadcast_to((upper > -10.0 * B / K - cell)[:, None, None], (res, res, res)))


def frame(r):
    return r.render(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "depth", "acc"))


def run(name, coarse, fine, arms):
    """arms: (label, function that puts the renderer into the arm's state); the first is the baseline."""
    r = nwe_amd.Renderer(0)
    r.set_network(0, coarse)
    r.set_network(1, fine)
    r.set_sampling(64, 128)
    ms, ran, rgb = {a: [] for a, _ in arms}, {}, {}
    full = 0
    for rep in range(3):
        for label, enter in arms:
            enter(r)
            for i in range(3):      # one launch to warm up, two timed
                out = frame(r)
                if i > 0:
                    ms[label].append(r.last_kernel_ms())
            ran[label], full = r.last_ray_evaluations()
            rgb[label] = out["rgb"]
            g = r.occupancy
            print(f"{name} {label} rep {rep}: kernel {ms[label][-2]:.2f} / {ms[label][-1]:.2f} ms, evaluations {ran[label]} of {full} "
                  f"({100.0 * ran[label] / full:.1f} %), occupied {'-' if g is None else format(g['occupied'], '.3f')}", flush=True)
    base_label = arms[0][0]
    base = statistics.median(ms[base_label])
    for label, _ in arms[1:]:
        t = statistics.median(ms[label])
        saved_t, saved_e = 1.0 - t / base, 1.0 - ran[label] / full
        d = (rgb[label] - rgb[base_label]).abs()
        mse = float((d.double() ** 2).mean())
        psnr = "inf" if mse == 0 else f"{-10.0 * np.log10(mse):.1f}"
        ratio = f", time saved per evaluation saved {saved_t / saved_e:.2f}" if saved_e > 0 else ""
        print(f"== {name} {label}: median {t:.2f} ms vs {base:.2f} ms ({100 * saved_t:+.1f} % time saved), {100 * saved_e:.1f} % of the "
              f"evaluations saved{ratio}; max |d rgb| {float(d.max()):.2e}, rays above 1e-4 {100 * float((d.max(-1).values > 1e-4).float().mean()):.2f} %, "
              f"PSNR {psnr} dB", flush=True)
    r.close()


def all_set(res):
    return lambda r: r.set_occupancy(np.ones((res, res, res), bool), LO, HI, res)


def built(dilate):
    return lambda r: r.build_occupancy(LO, HI, 128, probes=2, threshold=0.0, dilate=dilate)


bench = synthetic.make_state_dict(1000, 8, 256), synthetic.make_state_dict(1001, 8, 256)
run("ask", *bench, (("none", lambda r: r.clear_occupancy()), ("all-set 128", all_set(128)), ("all-set 256", all_set(256))))
run("built", *bench, (("none", lambda r: r.clear_occupancy()), ("dilate 0", built(0)), ("dilate 1", built(1))))
run("slab", slab(2000), slab(2001), (("none", lambda r: r.clear_occupancy()), ("exact 128", lambda r: r.set_occupancy(slab_bits(128), LO, HI, 128))))
