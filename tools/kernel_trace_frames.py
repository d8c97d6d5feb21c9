"""Per-frame summary of a rocprofv3 kernel trace of bench.py (rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME --
python bench.py --gpus 1 --steps K --warmup W): the table LABBOOK R18.1 / R19.1 quote.  No GPU.

A frame starts at a raygen_kernel launch; only frames with a successor are counted (the last one has no end).  Per frame: span (start of
its raygen to the start of the next), summed kernel time, idle time between consecutive launches; per kernel: launches per frame, mean and
median microseconds per launch, milliseconds per frame.  Warm-up frames are dropped by keeping the last `frames` complete ones (19 of
--steps 20: the last timed frame has no successor), and of those the ones with the median launch count.

  python tools/kernel_trace_frames.py <kernel_trace.csv> [label] [frames=19]
"""
import csv
import statistics
import sys


def short(name):
    """the kernel's own name: no return type, template arguments or parameter list"""
    return name.replace("void ", "").split("<")[0].split("(")[0]


def main(path, label, frames):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if "raygen_kernel" in r[2]]
    spans = [(starts[k], starts[k + 1]) for k in range(len(starts) - 1)][-frames:]
    if not spans:
        sys.exit("no complete frame in the trace")
    n_launch = statistics.median(b - a for a, b in spans)
    spans = [(a, b) for a, b in spans if b - a == n_launch]   # the timed frames all have the same launches
    span_ms, kern_ms, idle_us, per = [], [], [], {}
    for a, b in spans:
        fr = rows[a:b]
        span_ms.append((rows[b][0] - fr[0][0]) / 1e6)
        kern_ms.append(sum(e - s for s, e, _ in fr) / 1e6)
        idle_us.append(sum(max(0, fr[i + 1][0] - fr[i][1]) for i in range(len(fr) - 1)) / 1e3)
        for s, e, n in fr:
            per.setdefault(n, []).append((e - s) / 1e3)
    print(f"== {label}: {len(spans)} frames, launches per frame {int(n_launch)}")
    print(f"   frame span ms median {statistics.median(span_ms):.3f} (min {min(span_ms):.3f} max {max(span_ms):.3f}); kernel time ms median "
          f"{statistics.median(kern_ms):.3f}; idle us per frame median {statistics.median(idle_us):.1f} (max {max(idle_us):.1f})")
    for n, us in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print(f"   {n:<60s} launches/frame {len(us) / len(spans):5.1f}  us/launch mean {statistics.mean(us):9.1f} median "
              f"{statistics.median(us):9.1f}  ms/frame {sum(us) / len(spans) / 1e3:8.3f}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else sys.argv[1], int(sys.argv[3]) if len(sys.argv) > 3 else 19)
