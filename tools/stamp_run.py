"""Diagnostic: where a sample iteration spends its cycles (needs the -DNWE_STAMPS build of the kernel, NWE_LIB), and the
clock the kernel really runs at: d(s_memtime) / d(s_memrealtime) x 100 MHz per wave, median over the waves of the last of
several back-to-back launches (MI355X_MICROARCH.md, DVFS give-back item 6).
    NWE_LIB=.../exp/libnwe_STAMPS.so python3 tools/stamp_run.py [H W [warm-up seconds]]
    NWE_LIB=.../exp/libnwe_STAMPS.so python3 tools/stamp_run.py --xcd [H W [warm-up seconds]]
--xcd: the frame under the plan the product takes (for 800x800 the hybrid one: packets, then the ragged round sample-split)
and, per XCD, what it ran and when it finished - the timeline of the LAST frame of the warm-up loop.  The stamped kernels
are the full (not LEAN) instantiations: read the XCDs against each other, not the frame's length."""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
torch.cuda.init()
argv = [a for a in sys.argv[1:] if a != "--xcd"]
XCD = "--xcd" in sys.argv[1:]
H, W = (int(argv[0]), int(argv[1])) if len(argv) > 1 else ((800, 800) if XCD else (128, 256))
WARM_S = float(argv[2]) if len(argv) > 2 else 0.0
ROW = 14                       # kStampWords (csrc/nwe_device.h); the row layout is in include/nwe.h
n_rays = H * W
cus = torch.cuda.get_device_properties(0).multi_processor_count
nw = (n_rays + 127) // 128 * 4 + ((n_rays + 31) // 32 * 4 if XCD else 0)   # --xcd: room for any plan's rows
buf = torch.zeros(nw * ROW, dtype=torch.int64, device="cuda")
import nwe_amd
r = nwe_amd.Renderer(0)
r._lib.nwe_debug_set_stamps(r._ctx, buf.data_ptr())
if not XCD:
    r.debug_set_decomposition(0)   # the cycle split below is read over workgroups of four packets
r.set_network(0, nwe_amd.synthetic.make_state_dict(1000, 8, 256)); r.set_network(1, nwe_amd.synthetic.make_state_dict(1001, 8, 256))
r.set_sampling(64, 128)
fx, fy, cx, cy = nwe_amd.pinhole_intrinsics(H, W)
pose = np.array([[0.8660254, 0, 0.5, 0], [-0.5, 0, 0.8660254, -0.76157], [0, -1, 0, 0.5], [0, 0, 0, 1]], np.float32)
import time
t_end = time.time() + WARM_S
n_warm = 0
while n_warm < 2 or time.time() < t_end:          # back-to-back launches: the die reaches its power-capped steady state
    out = r.render(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb",))
    n_warm += 1
    if n_warm % 4 == 0:
        torch.cuda.synchronize()
torch.cuda.synchronize()
if XCD:   # one more frame into a cleared buffer: every row read below is this frame's
    buf.zero_()
    out = r.render(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb",))
    n_warm += 1
    torch.cuda.synchronize()
print("launches", n_warm, "frame", H, "x", W)
print("kernel ms", r.last_kernel_ms())
raw = buf.cpu().numpy().reshape(nw, ROW)
st = raw.astype(np.float64)
st = st[st[:, 4] > 0]
clk = st[:, 4] / st[:, 8] * 0.1
print(f"in-kernel clock: median {np.median(clk):.3f} GHz (p10 {np.quantile(clk, 0.1):.3f}, p90 {np.quantile(clk, 0.9):.3f}) over {len(clk)} waves; "
      f"wave lifetime median {np.median(st[:, 8]) / 100:.0f} us")
if not XCD:
    names = ["ray/depth/gamma(x)", "initial sync + prologue reads", "mlp_eval", "composite + stores", "whole kernel",
             "  tiles: start -> barrier wait", "  tiles: wait + barrier", "  tiles: barrier -> end"]
    tot = st[:, 4].mean()
    for i, n in enumerate(names):
        print(f"{n:32s} {st[:, i].mean() / 256:10.0f} cycles/iteration  {st[:, i].mean() / tot:6.1%}")
    sys.exit(0)

# ---- per-XCD timeline ----
plan = r._lib.nwe_debug_last_plan(r._ctx)
per = {0: 128, 1: 32}
if plan == 2:
    first = n_rays // 128 // cus * cus * 128                     # plan_launch: the complete rounds of packet workgroups
    launches = [("packets", first // 128), ("split", (n_rays - first + 31) // 32)]
else:
    launches = [("packets" if plan == 0 else "split", (n_rays + per[plan] - 1) // per[plan])]
q = r.debug_last_queue()
row0 = 0
for i, (name, items) in enumerate(launches):                     # a row per wave of a work item, whichever workgroup of the grid took it
    launches[i] = (name, row0, items)
    row0 += items
print("plan", plan, "work queue mode", r.debug_get_work_queue(), q, "launches (name, first work item's row, work items)", launches, "CUs", cus)
# one record per workgroup: XCD, CU (shader engine / array / CU fields of HW_ID: bits 8-15), start, end, clock
def workgroups(row0, wgs):
    w = raw[row0 * 4:(row0 + wgs) * 4].reshape(wgs, 4, ROW)
    ok = (w[:, :, 4] > 0).all(axis=1)
    w = w[ok]
    xcc = (w[:, 0, 10] & 0xf).astype(int)
    cu = ((w[:, 0, 10] >> 32) >> 8 & 0xff).astype(int)
    start = w[:, :, 12].min(axis=1).astype(np.float64) / 100.0    # us on the 100 MHz clock
    end = w[:, :, 13].max(axis=1).astype(np.float64) / 100.0
    clock = (w[:, :, 4].astype(np.float64) / w[:, :, 8] * 0.1).mean(axis=1)
    return dict(xcc=xcc, cu=cu, start=start, end=end, clock=clock, missing=int((~ok).sum()), item=w[:, 0, 11])
recs = [(name, workgroups(row0, wgs)) for name, row0, wgs in launches]
frame0 = min(rc["start"].min() for _, rc in recs)
frame1 = max(rc["end"].max() for _, rc in recs)
print(f"frame on the 100 MHz clock: {(frame1 - frame0) / 1000:.3f} ms from the first workgroup's start to the last one's end")
for name, rc in recs:
    print(f"launch {name}: {len(rc['xcc'])} work items rendered (without stamps: {rc['missing']}), first start +{(rc['start'].min() - frame0) / 1000:.3f} ms, "
          f"last end +{(rc['end'].max() - frame0) / 1000:.3f} ms")
print("wgs = work items rendered; last end = the XCD's last workgroup of the launch, from the launch's first start; idle = the share of the")
print("XCD's CU-time, over the frame, between a CU's last end of this launch and the start of the CU's next workgroup of the frame")
print("(the frame's end where there is none): what static dealing leaves on the table")
print("XCD | " + " | ".join(f"{name}: wgs  CUs  clock GHz  wg life ms  last end ms  ms per round   idle" for name, _ in recs) + " | idle tail")
rounds_ms = []
for x in range(8):
    cells = []
    last_by_cu = {}
    for name, rc in recs:
        m = rc["xcc"] == x
        if not m.any():
            cells.append(f"{name}: none")
            continue
        life = np.median(rc["end"][m] - rc["start"][m]) / 1000
        t0 = rc["start"].min()
        last = (rc["end"][m].max() - t0) / 1000
        ncu = len(set(rc["cu"][m]))
        per_round = last / np.ceil(m.sum() / ncu)
        if name == "packets": rounds_ms.append(per_round)
        # per CU: from its last end of this launch to its next start of the frame, in any launch
        gap = 0.0
        for c in set(rc["cu"][m]):
            e = rc["end"][m][rc["cu"][m] == c].max()
            later = [rc2["start"][(rc2["xcc"] == x) & (rc2["cu"] == c) & (rc2["start"] >= e)] for _, rc2 in recs]
            later = np.concatenate(later)
            gap += (later.min() if len(later) else frame1) - e
        cells.append(f"{name}: {m.sum():5d} {ncu:3d} {np.median(rc['clock'][m]):9.3f} {life:10.3f} {last:11.3f} {per_round:10.3f} {gap / (ncu * (frame1 - frame0)):6.2%}")
        for c, e in zip(rc["cu"][m], rc["end"][m]):
            last_by_cu[c] = max(last_by_cu.get(c, 0.0), e)
    idle = sum(frame1 - e for e in last_by_cu.values()) / (max(len(last_by_cu), 1) * (frame1 - frame0))
    print(f"{x:3d} | " + " | ".join(cells) + f" | {idle:6.2%}")
if len(rounds_ms) == 8:
    print("packet round times per XCD for tools/queue_model.py (ms):", " ".join(f"{v:.4f}" for v in rounds_ms))
