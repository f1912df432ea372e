#!/usr/bin/env python
"""Time contribs.PlaneWaveNeurons beside GridCells on the same build, in one process, at the flagship batch: 4096 agents x
1024 cells, one [n][B] rate row (16.8 MB) per step of Agent.simulate().

    python tools/plane_wave_time.py [--steps 128] [--repeats 7] [--warmup 2] [--agents 4096] [--cells 1024]
                                    [--out profiles/plane_wave_time.txt]

What is timed (HIP events around the call; the figure of a repeat is its mean per step, the figure reported is the MEDIAN
over the repeats, min and max beside it — DESIGN.md 6, the method of tools/theta_time.py): `Agent.simulate(steps)` with the
population as the agent's only one, so it leads the row-following rate kernel (the one-kernel form; the form each call took is
recorded).  The two populations take turns, repeat by repeat, so that a drift of the device's clocks lands on both.  Neither
keeps a history or draws spikes (a ring of rows is overwritten: the store stream alone).  One JSON line per population and a
last line with the comparison the change was made against: PlaneWaveNeurons (one cosine per rate) is expected to be no
slower than GridCells (three) by more than GridCells' own max - min spread in the run."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ratinabox_amd as riab  # noqa: E402
from ratinabox_amd.contribs.PlaneWaveNeurons import PlaneWaveNeurons  # noqa: E402


def make(kind, agents, cells):
    np.random.seed(1)
    ag = riab.Agent(riab.Environment({}), {"n_agents": agents, "dt": 0.01, "seed": 3, "save_history": False})
    p = {"n": cells, "save_history": False, "save_spikes": False}
    N = PlaneWaveNeurons(ag, p) if kind == "plane_wave" else riab.GridCells(ag, p)
    return ag, N


def timed(ag, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ag.simulate(steps)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5, "at least 5 repeats each"
    kinds = ("plane_wave", "grid")
    worlds = {k: make(k, a.agents, a.cells) for k in kinds}
    us = {k: [] for k in kinds}
    forms = {k: set() for k in kinds}
    for r in range(a.warmup + a.repeats):
        for k in kinds:                      # alternating
            ag, _N = worlds[k]
            t = timed(ag, a.steps)
            if r >= a.warmup:
                us[k].append(t)
                forms[k].add(ag.last_rate_stage_form())
    nbytes = 4 * a.cells * a.agents
    lines = []
    for k in kinds:
        med = statistics.median(us[k])
        lines.append(json.dumps({"population": "PlaneWaveNeurons" if k == "plane_wave" else "GridCells", "what": "Agent.simulate",
                                 "agents": a.agents, "cells": a.cells, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
                                 "us_per_step_median": round(med, 3), "us_min": round(min(us[k]), 3), "us_max": round(max(us[k]), 3),
                                 "spread_us": round(max(us[k]) - min(us[k]), 3), "row_bytes": nbytes,
                                 "TB_per_s_of_row": round(nbytes / med * 1e-6, 3), "rate_stage_form": sorted(map(str, forms[k]))}))
        print(lines[-1], flush=True)
    pw, gc = statistics.median(us["plane_wave"]), statistics.median(us["grid"])
    spread = max(us["grid"]) - min(us["grid"])
    lines.append(json.dumps({"plane_wave_minus_grid_us_per_step": round(pw - gc, 3), "grid_spread_us": round(spread, 3),
                             "plane_wave_not_slower_than_grid_by_more_than_its_spread": bool(pw - gc <= spread)}))
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
