"""The asynchronous sparse frame against the synchronous one on the bench frame (800x800, 8x256, 64+128, a 128^3 grid baked as
tools/sparse_fine_ab.py bakes it), under that tool's protocol: arms alternating on one box, three repetitions of two timed frames
behind one that warms up, reported as median (min - max).

  parent sync    nwe_render_sparse of another checkout (--parent ROOT: a built tree of the parent commit), in a process of its own
  sync           nwe_render_sparse of this tree
  async          nwe_render_sparse_async
  grid           nwe_render_grid, the proposal alone: what the constant of the sparse call is measured against

Scenes: synthetic.room at min_weight 1e-2, 1e-3, 2 and -1, and the benchmark's random networks at 1e-3; dilate 1.
Per arm two times: the device span (nwe_last_sparse_ms / nwe_last_grid_ms) and the host wall time from the call to its return, with
the device idle when the call is made.  (The run that decided against a second chunk buffer on a side stream had two asynchronous
arms, profiles/r14_ab_sparse_async.txt; the tree has the one that was kept.)  Every repetition is a fresh process per checkout,
the parent's first, so the arms alternate and no process loads two libraries.  DESIGN.md section 5.9 quotes the result.
Usage on the GPU box: python tools/sparse_async_ab.py [--parent ROOT] [H W]."""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = (-16.0, -16.0, -16.0), (16.0, 16.0, 16.0)      # tools/sparse_fine_ab.py
RES = 128
CASES = (("room", 1e-2), ("room", 1e-3), ("room", 2.0), ("room", -1.0), ("bench", 1e-3))
REPS = 3


def child(root, H, W):
    """One repetition of every arm this checkout has; prints one JSON line per arm and case."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import nwe_amd
    from nwe_amd import synthetic as S
    from nwe_amd.handler import NeRFReplicaInferenceHandler as Handler

    pose = np.array([[0.8660254, 0, 0.5, 0], [-0.5, 0, 0.8660254, -0.76157], [0, -1, 0, 0.5], [0, 0, 0, 1]], np.float32)
    fx, fy, cx, cy = nwe_amd.pinhole_intrinsics(H, W)
    cam = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0)
    has_async = hasattr(nwe_amd.Renderer, "debug_last_sparse_host_waits")

    def renderer(sds):
        r = nwe_amd.Renderer(0)
        r.set_network(0, sds[0]); r.set_network(1, sds[1])
        r.set_sampling(64, 128)
        total = RES ** 3
        raw = torch.empty((total, 4), dtype=torch.float32, device=r.device)
        for start in range(0, total, 1 << 20):
            count = min(1 << 20, total - start)
            pts = Handler.grid_centres(LO, HI, (RES,) * 3, start, count, device=r.device)[None]
            acc = None
            for d in Handler._AXIS_DIRECTIONS:
                row = r.query_points(pts, torch.tensor([d], dtype=torch.float32, device=r.device), outputs=("raw",))["raw"][0]
                acc = row if acc is None else acc + row
            raw[start:start + count] = acc / 6.0
        r.set_radiance_grid(raw.reshape(RES, RES, RES, 4), LO, HI)
        return r

    def measure(call, last_ms):
        device, host = [], []
        for i in range(3):      # one frame to warm up, two timed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if i > 0:
                device.append(last_ms()); host.append(1e3 * (t1 - t0))
        return device, host

    scenes = {"room": (S.room(S.make_state_dict(1000, 8, 256)), S.room(S.make_state_dict(1001, 8, 256))),
              "bench": (S.make_state_dict(1000, 8, 256), S.make_state_dict(1001, 8, 256))}
    for scene, sds in scenes.items():
        ctx = renderer(sds)
        arms = [("sync" if has_async else "parent sync", ctx, {})]
        if has_async:
            arms.append(("async", ctx, dict(asynchronous=True)))
        for s, mw in CASES:
            if s != scene:
                continue
            for label, r, kw in arms:
                device, host = measure(lambda: r.render_sparse(pose, H, W, min_weight=mw, dilate=1, **cam, **kw), r.last_sparse_ms)
                print(json.dumps(dict(arm=label, scene=scene, min_weight=mw, device=device, host=host, samples=r.last_sparse_samples())), flush=True)
        if has_async:
            device, host = measure(lambda: ctx.render_grid(pose, H, W, **cam), ctx.last_grid_ms)
            print(json.dumps(dict(arm="grid", scene=scene, min_weight=None, device=device, host=host, samples=None)), flush=True)
        ctx.close()


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1], int(args[2]), int(args[3]))
    parent = None
    if args and args[0] == "--parent":
        parent, args = os.path.abspath(args[1]), args[2:]
    H, W = (int(args[0]), int(args[1])) if len(args) > 1 else (800, 800)
    rows = {}
    for rep in range(REPS):
        for root in ([parent] if parent else []) + [HERE]:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, str(H), str(W)], check=True,
                                 capture_output=True, text=True).stdout
            for line in out.splitlines():
                if not line.startswith("{"):
                    continue
                d = json.loads(line)
                key = (d["scene"], d["min_weight"], d["arm"])
                entry = rows.setdefault(key, dict(device=[], host=[], samples=d["samples"]))
                entry["device"] += d["device"]; entry["host"] += d["host"]
                print(f"rep {rep} {d['scene']} min_weight {d['min_weight']} {d['arm']}: device {d['device'][0]:.3f} / {d['device'][1]:.3f} ms, "
                      f"host {d['host'][0]:.3f} / {d['host'][1]:.3f} ms", flush=True)
    fmt = lambda v: f"{statistics.median(v):.3f} ({min(v):.3f} - {max(v):.3f})"
    for (scene, mw, arm), e in rows.items():
        share = "" if e["samples"] is None else f"; selected {e['samples'][0]} of {e['samples'][1]} = {e['samples'][0] / e['samples'][1]:.4f}"
        print(f"== {scene} min_weight {mw} {arm}: device ms {fmt(e['device'])}, host ms until the call returns {fmt(e['host'])}{share}", flush=True)


if __name__ == "__main__":
    main()
