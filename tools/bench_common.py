"""What the tools/*_bench.py files share: how a call is timed and how the result line leaves."""
import json
import os
import statistics

import torch


def time_calls(fn, warmup, steps):
    """the median over ``steps`` calls of the device time of one, events around each, after ``warmup`` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def write_line(res, out):
    """prints ``res`` as one JSON line and, if ``out`` names a file, writes the line there"""
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
