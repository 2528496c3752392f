"""The pixel list on the bench frame (800x800, 8x256, 64+128, f16x3): arms alternating in one process on one box, three repetitions
of two timed frames each (medians of six, device events), on the room (synthetic.room), on a dense_fog scene and on the
benchmark's random networks:

  (a) render          the ordinary frame (nwe_render)
  (b) rays            nwe_render_rays on the whole frame's rays, lean outputs: the parent's path for a list of pixels
  (c) pixels          nwe_render_pixels with the identity list: the same pixels on the list kernels - its yardstick is (b)
  (d) pixels shuffled (c) with a seeded random permutation of the list: what the hollow path loses when packets are scattered
  (e) pixels blocked  (c) with the list in 8x4-block order (nwe_debug_packet_pixels): the packets nwe_render itself forms
  (f) adaptive off    the adaptive frame, k = 2, tol_rgb 2/255, tol_depth 0.05, nwe_set_adaptive_pixel_lists off   (room only)
  (g) adaptive on     the same with the switch on                                                                  (room only)

Per arm the device time - nwe_last_kernel_ms, or the span of nwe_last_adaptive - as median (min - max) and its ratio to (a) and
to (b); whether (c), (d), (e) give the frame's bits (gathered at the list), and (g) the bits of (f).  DESIGN.md section 5.11 quotes it.
Usage on the GPU box: python tools/pixels_ab.py [H W [scene ...]] with scenes of room, fog, bench (default: all three)."""
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nwe_amd
from nwe_amd import _lib, synthetic

H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (800, 800)
SCENES = sys.argv[3:] or ["room", "fog", "bench"]
pose = np.array([[0.8660254, 0, 0.5, 0], [-0.5, 0, 0.8660254, -0.76157], [0, -1, 0, 0.5], [0, 0, 0, 1]], np.float32)
fx, fy, cx, cy = nwe_amd.pinhole_intrinsics(H, W)
CAM = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0)
ADAPTIVE = dict(k=2, tol_rgb=2 / 255, tol_depth=0.05)


def same(a, b):
    return bool(torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)))


def run(name, scene, sds):
    print(f"==== scene: {scene}", flush=True)
    r = nwe_amd.Renderer(0)
    r.set_network(0, sds[0]); r.set_network(1, sds[1])
    r.set_sampling(64, 128)
    rays = r.create_rays(pose, H, W, **CAM)
    n = H * W
    lists = {"identity": np.arange(n, dtype=np.int32), "shuffled": np.random.default_rng(17).permutation(n).astype(np.int32)}
    if H % 4 == 0 and W % 8 == 0:
        blocked = np.empty(n, np.int32)
        assert _lib.load().nwe_debug_packet_pixels(0, n, W, blocked.ctypes.data_as(C.c_void_p)) == _lib.NWE_OK
        lists["blocked"] = blocked
    dev_lists = {k: torch.from_numpy(v).to(r.device) for k, v in lists.items()}
    pixels = lambda which: (lambda: r.render_pixels(pose, H, W, dev_lists[which], outputs=("rgb",), **CAM))
    arms = [("(a) render", lambda: r.render(pose, H, W, outputs=("rgb",), **CAM), r.last_kernel_ms),
            ("(b) rays", lambda: r.render_rays(rays, outputs=("rgb",)), r.last_kernel_ms),
            ("(c) pixels", pixels("identity"), r.last_kernel_ms), ("(d) pixels shuffled", pixels("shuffled"), r.last_kernel_ms)]
    if "blocked" in lists:
        arms.append(("(e) pixels blocked", pixels("blocked"), r.last_kernel_ms))
    if name == "room":
        def adaptive(on):
            r.set_adaptive_pixel_lists(on)
            try:
                return r.render_adaptive(pose, H, W, **ADAPTIVE, **CAM)
            finally:
                r.set_adaptive_pixel_lists(False)
        arms += [("(f) adaptive off", lambda: adaptive(False), lambda: r.last_adaptive()["ms"]),
                 ("(g) adaptive on", lambda: adaptive(True), lambda: r.last_adaptive()["ms"])]
    dev, rgb, notes = {a[0]: [] for a in arms}, {}, {}
    for rep in range(3):
        for label, render, last_ms in arms:
            for i in range(3):      # one frame to warm up, two timed
                torch.cuda.synchronize()
                out = render()
                torch.cuda.synchronize()
                if i > 0:
                    dev[label].append(last_ms())
            rgb[label] = out["rgb"]
            if label.startswith("(c)") or label.startswith("(d)") or label.startswith("(e)"):
                notes[label] = f"path {r.last_pixels()['path']}"
            if label.startswith("(f)") or label.startswith("(g)"):
                c = r.last_adaptive()
                notes[label] = f"lattice {c['lattice']}, rendered {c['rendered']}, interpolated {c['interpolated']} of {c['pixels']}"
            print(f"{label} rep {rep}: device {dev[label][-2]:.3f} / {dev[label][-1]:.3f} ms", flush=True)
    frame = rgb["(a) render"]
    print(f"bits: (b) = (a): {same(rgb['(b) rays'], frame)}; (c) = (a): {same(rgb['(c) pixels'], frame)}; "
          f"(d) = (a) gathered: {same(rgb['(d) pixels shuffled'], frame[dev_lists['shuffled'].long()])}"
          + (f"; (e) = (a) gathered: {same(rgb['(e) pixels blocked'], frame[dev_lists['blocked'].long()])}" if "blocked" in lists else "")
          + (f"; (g) = (f): {same(rgb['(g) adaptive on'], rgb['(f) adaptive off'])}" if name == "room" else ""))
    med = {a: statistics.median(v) for a, v in dev.items()}
    for label in dev:
        print(f"== {label}: device median {med[label]:.3f} ms ({min(dev[label]):.3f} - {max(dev[label]):.3f}, spread {max(dev[label]) - min(dev[label]):.3f}); "
              f"{med[label] / med['(a) render']:.4f} x (a), {med[label] / med['(b) rays']:.4f} x (b)" + (f"; {notes[label]}" if label in notes else ""), flush=True)
    gain, spread = med["(b) rays"] - med["(c) pixels"], max(max(dev[k]) - min(dev[k]) for k in ("(b) rays", "(c) pixels"))
    print(f"== (b) - (c) = {gain:.3f} ms against a spread of {spread:.3f} ms: (c) is {'faster' if gain > spread else 'NOT faster'} than (b) by more than the run's spread",
          flush=True)
    r.close()


def main():
    S = synthetic
    scenes = {"room": ("room (walls at +-3, both networks)", lambda: (S.room(S.make_state_dict(1000, 8, 256)), S.room(S.make_state_dict(1001, 8, 256)))),
              "fog": ("dense_fog(0.5, 3.0) fine under a thin_fog coarse network",
                      lambda: (S.thin_fog(S.make_state_dict(1000, 8, 256)), S.dense_fog(S.make_state_dict(1001, 8, 256), 0.5, 3.0))),
              "bench": ("bench (random networks)", lambda: (S.make_state_dict(1000, 8, 256), S.make_state_dict(1001, 8, 256)))}
    for name in SCENES:
        title, make = scenes[name]
        run(name, title, make())


if __name__ == "__main__":
    main()
