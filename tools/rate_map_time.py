#!/usr/bin/env python
"""Time Neurons.get_rate_map_tensor (csrc/riab_ratemap.hip) on a long recorded run, beside a plain reduction that reads
the same bytes: 4096 agents x 1024 PlaceCells x 256 recorded steps on a 20 x 20 grid, about 4.3 GB of fp32 rates.

    python tools/rate_map_time.py [--agents 4096] [--cells 1024] [--steps 256] [--calls 4] [--repeats 7]
                                  [--host-agents 256] [--out profiles/rate_map_time.txt]

The run is recorded by `--calls` simulate() calls, so the history spans that many chunks.  Timed with HIP events around
the whole call, after two warm-up calls; reported: the MEDIAN over the repeats, min and max beside it.
  rate map     get_rate_map_tensor(): bin ids + occupancy (stage A), weighted sums (stage B), slab reduce, finish
  occupancy    Agent.get_position_heatmap_tensor(): stage A alone, on the same rows
  torch.sum    the yardstick: `chunk[:filled].sum()` over the same rate chunks (reads the same bytes, writes nothing)
  host route   at `--host-agents` agents (a size it can finish): history["firingrate"] (stack, copy to the host) plus
               utils.bin_data_for_histogramming per cell; host clock, once
bytes = 4 n B T, the rate rows (the trajectory rows and the bin ids are 1 / n of that and not counted).  One JSON line
per figure."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ratinabox_amd as riab  # noqa: E402
from ratinabox_amd import utils  # noqa: E402


def events(fn, repeats):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def record(agents, cells, steps, calls):
    np.random.seed(1)
    ag = riab.Agent(riab.Environment({}), {"n_agents": agents, "dt": 0.01, "seed": 3})
    pcs = riab.PlaceCells(ag, {"n": cells, "wall_geometry": "euclidean", "save_spikes": False})
    per = max(1, steps // calls)
    done = 0
    while done < steps:
        k = min(per, steps - done)
        ag.simulate(k)
        done += k
    torch.cuda.synchronize()
    return ag, pcs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--bin-size", type=float, default=0.05)
    ap.add_argument("--host-agents", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def report(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    ag, pcs = record(a.agents, a.cells, a.steps, a.calls)
    h = pcs._hist_fr
    rows = len(h) - 1                                     # (the reference's slice leaves the last row out)
    nbytes = 4 * a.cells * ag._Bp * rows
    common = dict(agents=a.agents, cells=a.cells, rows=rows, chunks=len(h.chunks), bin_size=a.bin_size, repeats=a.repeats,
                  rate_bytes=nbytes)

    def yardstick():
        left, tot = rows, None
        for c, f in zip(h.chunks, h.filled):
            k = min(f, left)
            if k > 0:
                s = c[:k].sum()
                tot = s if tot is None else tot + s
                left -= k
        return tot

    figures = {}
    for name, fn in (("rate map", lambda: pcs.get_rate_map_tensor(bin_size=a.bin_size)),
                     ("torch.sum", yardstick),
                     ("occupancy", lambda: ag.get_position_heatmap_tensor(dx=a.bin_size)),
                     ("rate map (again)", lambda: pcs.get_rate_map_tensor(bin_size=a.bin_size)),
                     ("torch.sum (again)", yardstick)):
        ms = events(fn, a.repeats)
        med = statistics.median(ms)
        figures[name] = med
        report(what=name, ms_median=round(med, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
               TB_per_s_of_rates=round(nbytes / med * 1e-9, 3), **common)
    report(what="ratio", rate_map_over_torch_sum=round(min(figures["rate map"], figures["rate map (again)"]) /
                                                       min(figures["torch.sum"], figures["torch.sum (again)"]), 3), **common)
    del ag, pcs, h
    torch.cuda.empty_cache()

    # the host route, at a size it can finish
    ag, pcs = record(a.host_agents, a.cells, a.steps, a.calls)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fr = pcs.history["firingrate"]
    pos = ag.history["pos"]
    t1 = time.perf_counter()
    sl = ag.get_history_slice(None, None)
    p = pos[sl].reshape(-1, 2).astype(np.float64)
    out = [utils.bin_data_for_histogramming(p, ag.Environment.extent, a.bin_size, weights=fr[sl][:, c].reshape(-1).astype(np.float64),
                                            norm_by_bincount=True) for c in range(a.cells)]
    t2 = time.perf_counter()
    dev = events(lambda: pcs.get_rate_map_tensor(bin_size=a.bin_size), a.repeats)
    got = pcs.get_rate_map(bin_size=a.bin_size)[0]
    report(what="host route", agents=a.host_agents, cells=a.cells, rows=len(p) // a.host_agents,
           fetch_s=round(t1 - t0, 3), binning_s=round(t2 - t1, 3), total_s=round(t2 - t0, 3),
           device_ms_median=round(statistics.median(dev), 3), max_abs_difference=float(np.abs(np.array(out) - got).max()))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
