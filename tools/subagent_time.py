#!/usr/bin/env python
"""Time contribs.SubAgent's DumbAgent and ReplayAgent at the flagship batch: 4096 agents x 1024 PlaceCells, dt 10 ms,
default parameters.

    python tools/subagent_time.py [--steps 200] [--repeats 5] [--agents 4096] [--cells 1024] [--timeout 240]
                                  [--out profiles/subagent_time.txt]

What is timed (HIP events round the loop, so the host's per-call work is in it where the device waits for it; the figure
of a repeat is its mean per step, the figure reported is the MEDIAN over the repeats, min and max beside it; 60 steps of
warm-up first):
  lead      Lead.update(); PCs.update()                   PCs on the lead, eager (a SubAgent has no plan either)
  dumb      Lead.update(); Dumb.update(); PCs.update()    PCs on a DumbAgent
  replay    Lead.update(); Rep.update(); PCs.update()     PCs on a ReplayAgent; also the sham agent's steps per update:
            the mean over the lanes inside a replay, and the mean of the largest count of an update (the trips of the
            loop in the slowest wave, which is what an update waits for)
Every variant runs in a process of its own under a time limit (a variant that fails or runs out of time ends the tool)
and prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

VARIANTS = ("lead", "dumb", "replay")


def events(torch, fn, repeats, steps):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / steps)
    return out


def run_variant(a):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ratinabox_amd as riab
    from ratinabox_amd.contribs.SubAgent import DumbAgent, ReplayAgent

    np.random.seed(1)
    lead = riab.Agent(riab.Environment({}), {"n_agents": a.agents, "dt": 0.01, "seed": 3, "save_history": False})
    lead._auto_enabled = False
    sub = {"lead": None, "dumb": DumbAgent, "replay": ReplayAgent}[a.variant]
    sub = sub(lead, {"save_history": False}) if sub else None
    pcs = riab.PlaceCells(sub or lead, {"n": a.cells, "wall_geometry": "euclidean", "save_history": False})
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")   # lanes in replay, their steps, largest count, updates

    def run(n):
        for _ in range(n):
            lead.update()
            if sub is not None:
                sub.update()
            if a.variant == "replay":
                steps = sub.replay_steps_taken[:a.agents]
                acc[0] += (steps > 0).sum()
                acc[1] += steps.sum()
                acc[2] += steps.max()
                acc[3] += 1
            pcs.update()

    run(60)
    torch.cuda.synchronize()
    acc.zero_()
    us = events(torch, lambda: run(a.steps), a.repeats, a.steps)
    info = {}
    if a.variant == "dumb":
        info = dict(sub.dumb_diagnostics)
    if a.variant == "replay":
        n_lanes, n_steps, n_max, n_calls = acc.cpu().tolist()
        info = dict(replay_steps_max=sub.replay_steps_max, sham_steps_per_stepping_lane=round(n_steps / max(n_lanes, 1), 2),
                    stepping_lanes_per_update=round(n_lanes / n_calls, 1), largest_count_per_update=round(n_max / n_calls, 2),
                    **sub.replay_diagnostics)
    med = statistics.median(us)
    print(json.dumps(dict({"what": a.variant, "agents": a.agents, "cells": a.cells, "steps": a.steps, "repeats": a.repeats,
                           "us_median": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)}, **info)),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds a variant may take")
    ap.add_argument("--variant", choices=VARIANTS, default=None, help="run this variant in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.variant:
        return run_variant(a)
    lines = []
    for v in VARIANTS:
        cmd = [sys.executable, os.path.abspath(__file__), "--variant", v, "--steps", str(a.steps), "--repeats", str(a.repeats),
               "--agents", str(a.agents), "--cells", str(a.cells)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"variant {v} did not finish within {a.timeout:.0f} s: nothing more is started")
        if r.returncode != 0:
            sys.exit(f"variant {v} ended with status {r.returncode}: nothing more is started")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        lines.append(line)
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
