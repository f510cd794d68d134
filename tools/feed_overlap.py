"""Copy / kernel overlap of a fed run, from the CSV output of
`rocprofv3 --kernel-trace --memory-copy-trace -f csv -d <dir> -o feed -- python tools/feed_bench.py ...`:

    python tools/feed_overlap.py <dir>/feed_kernel_trace.csv <dir>/feed_memory_copy_trace.csv

For every host-to-device copy of 2 - 7 ms (a fed batch's images or scans at B = 128; the 7.5 ms single copies of the ceiling
leg are left out) it prints when it starts, the idle time of the link before it and the kernels that ran in that gap, how
many kernels overlap the copy and for what fraction of its time at least one kernel runs, then the total over those copies.
Copies back to back (gap ~0) whose kernels overlap them are the steady state; a long gap is the host filling the slots.
"""
import csv
import sys


def union_inside(intervals, s, e):
    iv = sorted((max(a, s), min(b, e)) for a, b in intervals if b > s and a < e)
    total, cur = 0, None
    for a, b in iv:
        if cur is None or a > cur[1]:
            if cur:
                total += cur[1] - cur[0]
            cur = [a, b]
        else:
            cur[1] = max(cur[1], b)
    if cur:
        total += cur[1] - cur[0]
    return total, len(iv)


def main(kernel_csv, copy_csv, lo_ms=2.0, hi_ms=7.0):
    ks = [(int(k["Start_Timestamp"]), int(k["End_Timestamp"])) for k in csv.DictReader(open(kernel_csv))]
    copies = [(int(c["Start_Timestamp"]), int(c["End_Timestamp"])) for c in csv.DictReader(open(copy_csv))
              if c["Direction"].endswith("HOST_TO_DEVICE")]
    copies = [c for c in copies if lo_ms * 1e6 < c[1] - c[0] < hi_ms * 1e6]
    copies.sort()
    busy = span = 0
    prev = None
    for s, e in copies:
        u, n = union_inside(ks, s, e)
        busy += u
        span += e - s
        gap = (s - prev) / 1e6 if prev is not None else 0.0
        in_gap = sum(1 for a, b in ks if prev is not None and a >= prev and b <= s)
        print("H2D at %8.2f ms, %.2f ms long; link idle %6.2f ms before it (%2d kernels there); %2d kernels overlap it, active %3.0f %%"
              % ((s - copies[0][0]) / 1e6, (e - s) / 1e6, gap, in_gap, n, 100.0 * u / (e - s)))
        prev = e
    print("%d input copies, %.1f ms; kernels active during %.1f ms of them (%.0f %%)" % (len(copies), span / 1e6, busy / 1e6,
                                                                                      100.0 * busy / max(span, 1)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
