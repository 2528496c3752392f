"""Same work, less idling: counters of the bench frame per arm of the work-queue A/B.  Each arm is a directory of rocprofv3 --pmc
passes over bench.py (one pass per counter set, no tracing; counters per frame = summed over the launches of a frame, as
tools/r03_profile_summary.py counts them) with the bench line of each pass beside it as <pass>.json.
    python3 tools/queue_pmc_summary.py <dir>/pmc_static <dir>/pmc_queue
Under --pmc the runtime runs one kernel at a time: the second launch of the hybrid plan does NOT backfill the first in these
passes, so they show the queue's part alone; the frame time of the real thing is tools/ab_bench.sh's."""
import glob, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from r03_profile_summary import counters

for arm in sys.argv[1:]:
    allc, kms = {}, {}
    for d in sorted(glob.glob(f"{arm}/pass_*")):
        if not os.path.isdir(d):
            continue
        c, n = counters(d)
        allc.update(c)
        try:
            ms = json.loads(open(d + ".json").read().strip().splitlines()[-1])["roofline"]["kernel_ms"]
        except Exception:   # noqa: BLE001
            ms = float("nan")
        for k in c:
            kms[k] = ms
        print(f"{arm} {os.path.basename(d)} ({n} frames, kernel {ms:.2f} ms per frame in that pass): " + ", ".join(f"{k} {v:.5g}" for k, v in c.items()))
    if "SQ_INSTS_MFMA" in allc:
        print(f"   SQ_INSTS_MFMA per frame {allc['SQ_INSTS_MFMA']:.5g}")
    if "SQ_BUSY_CU_CYCLES" in allc:
        print(f"   SQ_BUSY_CU_CYCLES per ms of kernel time {allc['SQ_BUSY_CU_CYCLES'] / kms['SQ_BUSY_CU_CYCLES']:.5g}")
    if "GRBM_GUI_ACTIVE" in allc:
        print(f"   GRBM_GUI_ACTIVE / 8 / kernel time = {allc['GRBM_GUI_ACTIVE'] / 8 / (kms['GRBM_GUI_ACTIVE'] * 1e-3) / 1e9:.3f} GHz effective clock")
    if "SQ_BUSY_CU_CYCLES" in allc and "GRBM_GUI_ACTIVE" in allc:
        print(f"   SQ_BUSY_CU_CYCLES / GRBM_GUI_ACTIVE = {allc['SQ_BUSY_CU_CYCLES'] / allc['GRBM_GUI_ACTIVE']:.4f} (separate passes)")
