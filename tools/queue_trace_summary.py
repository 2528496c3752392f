"""When the sample-split kernel of a frame started and ended relative to the packets kernel (rocprofv3 --kernel-trace CSV).
On the tail path both launches of a frame are render_mfma_tail_kernel: the first, with the larger grid, is the packets launch whose
surplus workgroups render the split items, the second the emptied sample-split launch behind it."""
import csv, glob, sys
rows = []
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "render_mfma" in r["Kernel_Name"]:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Grid_Size_X", "?"), r.get("Queue_Id", "?"), r.get("Stream_Id", "?")))
rows.sort()
def split(name):
    a = name.split("<", 1)[-1].split(",")
    return len(a) > 4 and a[4].strip() == "true"
pk = None
for i, (s, e, n, g, q, st) in enumerate(rows):
    if "render_mfma_tail_kernel" in n:
        # launches come in pairs, first then second, the second forked behind the first
        first = pk is None or len(pk) < 3
        if first:
            pk = (s, e, "tail-first")
            print(f"packets + tail: grid {g} queue {q} stream {st}: {(e - s) / 1e6:.3f} ms")
        else:
            print(f"  emptied split launch: grid {g} queue {q} stream {st}: starts {(s - pk[1]) / 1e6:+.3f} ms from the first launch's end, "
                  f"runs {(e - s) / 1e6:.3f} ms; frame {(e - pk[0]) / 1e6:.3f} ms")
            pk = None
        continue
    if not split(n):
        pk = (s, e)
        print(f"packets: grid {g} queue {q} stream {st}: {(e - s) / 1e6:.3f} ms")
    elif pk:
        print(f"  split: grid {g} queue {q} stream {st}: starts {(s - pk[0]) / 1e6:+.3f} ms after the packets kernel's start ({(s - pk[1]) / 1e6:+.3f} ms from its end), "
              f"runs {(e - s) / 1e6:.3f} ms, ends {(e - pk[1]) / 1e6:+.3f} ms from the packets kernel's end; frame {(max(e, pk[1]) - pk[0]) / 1e6:.3f} ms")
