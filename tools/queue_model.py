"""Model: what dealing a frame's workgroups from a queue could save over the static dealing of the hardware (workgroup b of
a launch goes to XCD (b + c) mod 8, an eighth of the launch each whatever pace an XCD runs at).  CPU only.
    python3 tools/queue_model.py r0 r1 r2 r3 r4 r5 r6 r7     per-XCD times of one round of packet workgroups (any unit),
                                                              e.g. the last line of `tools/stamp_run.py --xcd`
    python3 tools/queue_model.py --spread 0.03 [--draws 200]  round times drawn uniformly in +-spread, mean gains and the worst
The frame: 4864 packet workgroups of cost 1 round and 544 sample-split workgroups of cost 0.241 (4.41 ms against 18.31 ms,
profiles/r03_pmc_summary.txt) on 8 XCDs of 32 CUs, one workgroup per CU at a time; a CU of XCD x runs an item of cost c in
c * r[x].  Three ways to hand them out:
    static          launch by launch, an eighth of each launch per XCD, 32 at a time
    queue           launch by launch, every free CU takes the launch's next item
    queue+backfill  one list, packets first: a free CU takes a split item as soon as the packets have run out"""
import heapq, sys
import numpy as np

N_PACKET, N_SPLIT, C_SPLIT, XCDS, CUS = 4864, 544, 0.241, 8, 32

def static_launch(r, n, cost):
    per_xcd = n // XCDS + (1 if n % XCDS else 0)
    return max(-(-per_xcd // CUS) * cost * rx for rx in r)

def queue_run(r, items, t0=0.0):
    """items: costs in the order they are taken; every CU free at t0.  Returns the time the last one ends."""
    free = [(t0, x * CUS + c) for x in range(XCDS) for c in range(CUS)]
    heapq.heapify(free)
    end = t0
    for cost in items:
        t, cu = heapq.heappop(free)
        t += cost * r[cu // CUS]
        end = max(end, t)
        heapq.heappush(free, (t, cu))
    return end

def frame_times(r):
    static = static_launch(r, N_PACKET, 1.0) + static_launch(r, N_SPLIT, C_SPLIT)
    queue = queue_run(r, [C_SPLIT] * N_SPLIT, queue_run(r, [1.0] * N_PACKET))
    backfill = queue_run(r, [1.0] * N_PACKET + [C_SPLIT] * N_SPLIT)
    return static, queue, backfill

def main():
    a = sys.argv[1:]
    if a and a[0] == "--spread":
        spread = float(a[1])
        draws = int(a[a.index("--draws") + 1]) if "--draws" in a else 200
        rng = np.random.default_rng(0)
        gq, gb = [], []
        for _ in range(draws):
            r = 1.0 + rng.uniform(-spread, spread, XCDS)
            r *= np.mean(1.0 / r)                     # one aggregate throughput in every draw
            s, q, b = frame_times(list(r))
            gq.append(1 - q / s); gb.append(1 - b / s)
        print(f"spread +-{spread:.1%}, {draws} draws: queue {np.mean(gq):+.2%} (worst {np.min(gq):+.2%}), "
              f"queue+backfill {np.mean(gb):+.2%} (worst {np.min(gb):+.2%})")
        return
    if len(a) != XCDS:
        sys.exit(__doc__)
    r = [float(v) for v in a]
    s, q, b = frame_times(r)
    mean = sum(r) / XCDS
    print("round times:", " ".join(f"{v:.4f}" for v in r), f"(spread {min(r) / mean - 1:+.2%} .. {max(r) / mean - 1:+.2%})")
    print(f"static          {s:10.4f}")
    print(f"queue           {q:10.4f}  {1 - q / s:+.2%}")
    print(f"queue+backfill  {b:10.4f}  {1 - b / s:+.2%}")

if __name__ == "__main__":
    main()
