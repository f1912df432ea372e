#!/usr/bin/env python
"""Time contribs.PhasePrecessingPlaceCells beside plain PlaceCells on the same build, at the flagship batch: 4096 agents x
1024 cells, one [n][B] rate row (16.8 MB) per step.

    python tools/theta_time.py [--steps 200] [--repeats 7] [--agents 4096] [--cells 1024] [--out profiles/theta_time.txt]

What is timed (HIP events; the figure of a repeat is its mean per step, the figure reported is the MEDIAN over the repeats,
min and max beside it):
  row kernel   the population's one-row launch (what update() / get_state() run: rate_kernel_wide, write-through stores),
               `steps` launches captured once in a graph and replayed — the device's time without the host's per-call work
  plan step    one closed-loop step of a native step plan holding the agent and that one population, `plan.step(steps)`:
               PlaceCells ride in the one-launch step (csrc/riab_step1.hip), PhasePrecessingPlaceCells are their own kernel
               behind the agent's (two launches per step)
Neither population keeps a history or draws spikes here (one row overwritten every step: the store stream alone).
Every variant prints one JSON line; bytes = 4 n B, the row."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ratinabox_amd as riab  # noqa: E402
from ratinabox_amd import _lib as L  # noqa: E402
from ratinabox_amd.contribs.PhasePrecessingPlaceCells import PhasePrecessingPlaceCells  # noqa: E402


def events(fn, repeats, steps):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / steps)
    return out


def make(kind, agents, cells, desc):
    np.random.seed(1)
    ag = riab.Agent(riab.Environment({}), {"n_agents": agents, "dt": 0.001, "seed": 3, "save_history": False})
    p = {"n": cells, "description": desc, "wall_geometry": "euclidean", "save_history": False, "save_spikes": False}
    N = PhasePrecessingPlaceCells(ag, dict(p, kappa=2.0)) if kind == "theta" else riab.PlaceCells(ag, p)
    return ag, N


def row_kernel(kind, a, desc):
    ag, N = make(kind, a.agents, a.cells, desc)
    ag.update()
    N.update()
    row = ag._last_row
    out = torch.empty((1, a.cells, ag._Bp), dtype=torch.float32, device="cuda")

    def one():
        N._modulated = True       # (the population at the agent, as update() runs it)
        N._launch(row[L.H_POS_X], row[L.H_POS_Y], row[L.H_HD_X], row[L.H_HD_Y], pos_ld=ag._Bp, T=1, B=ag._Bp, rates=out,
                  spikes=None, u_in=None, dt=0.001, step0=1)

    for _ in range(20):
        one()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(a.steps):
            one()
    g.replay()
    torch.cuda.synchronize()
    return events(g.replay, a.repeats, a.steps)


def plan_step(kind, a, desc):
    ag, N = make(kind, a.agents, a.cells, desc)
    plan = ag.make_step_plan(capacity=max(a.steps, 64))
    plan.step(20)
    torch.cuda.synchronize()
    us = events(lambda: plan.step(a.steps), a.repeats, a.steps)
    info = plan.info()
    plan.close()
    return us, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    nbytes = 4 * a.cells * a.agents
    for desc in ("gaussian", "gaussian_threshold"):
        for kind in ("place", "theta"):
            for what in ("row kernel", "plan step"):
                if what == "row kernel":
                    us, info = row_kernel(kind, a, desc), {}
                else:
                    us, info = plan_step(kind, a, desc)
                med = statistics.median(us)
                lines.append(json.dumps({"population": "PhasePrecessingPlaceCells" if kind == "theta" else "PlaceCells",
                                         "description": desc, "what": what, "agents": a.agents, "cells": a.cells, "steps": a.steps,
                                         "repeats": a.repeats, "us_per_step_median": round(med, 3), "us_min": round(min(us), 3),
                                         "us_max": round(max(us), 3), "row_bytes": nbytes,
                                         "TB_per_s_of_row": round(nbytes / med * 1e-6, 3),
                                         "fused_populations": info.get("fused_populations")}))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
