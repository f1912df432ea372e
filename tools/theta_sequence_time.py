#!/usr/bin/env python
"""Time contribs.SubAgent.ThetaSequenceAgent at the flagship batch: 4096 agents x 1024 PlaceCells, dt 2 ms.

    python tools/theta_sequence_time.py [--steps 200] [--repeats 5] [--agents 4096] [--cells 1024]
                                        [--out profiles/theta_sequence_time.txt]

What is timed (HIP events round the loop, so the host's per-call work is in it where the device waits for it; the figure
of a repeat is its mean per step, the figure reported is the MEDIAN over the repeats, min and max beside it):
  loop with sweep     Lead.update(); TS.update(); PCs.update()    PCs on the ThetaSequenceAgent (eager: a SubAgent has no plan)
  loop without        Lead.update(); PCs.update()                 PCs on the lead, the automatic step plan switched off, and on
  step kernel         riab_theta_sequence_step alone in its look-behind branch, the ring full and every lane past d_half, at
                      lookback 390 and 3906 (what dt 20 ms and 2 ms give): a bisection, so it must not grow like the lookback
  rollout kernel      riab_theta_sequence_rollout alone (Philox noise), from the lead's state
Every variant prints one JSON line."""
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
from ratinabox_amd.contribs.SubAgent import ThetaSequenceAgent  # noqa: E402


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


def build(a, sweep, auto=True, dt=0.002):
    np.random.seed(1)
    lead = riab.Agent(riab.Environment({}), {"n_agents": a.agents, "dt": dt, "seed": 3, "save_history": False})
    ts = ThetaSequenceAgent(lead, {"save_history": False}) if sweep else None
    pcs = riab.PlaceCells(ts if sweep else lead, {"n": a.cells, "wall_geometry": "euclidean", "save_history": False})
    lead._auto_enabled = auto
    return lead, ts, pcs


def loop(a, sweep, auto=True):
    lead, ts, pcs = build(a, sweep, auto)

    def run(n):
        for _ in range(n):
            lead.update()
            if sweep:
                ts.update()
            pcs.update()

    run(60)
    torch.cuda.synchronize()
    us = events(lambda: run(a.steps), a.repeats, a.steps)
    return us, ({} if ts is None else dict(rollouts=ts.n_rollouts, **ts.theta_diagnostics))


def step_kernel(a, n):
    lead, ts, _pcs = build(a, True, False)
    lead.update()
    # a full ring of `n` records that spans 0.4 m and a lead past d_half: every lane bisects its whole window, then
    # interpolates (lookback 390 is what dt 20 ms would give, 3906 is dt 2 ms)
    assert n <= ts.lookback
    Bp = ts._Bp
    d = torch.arange(n, dtype=torch.float64, device="cuda") * (0.4 / n)
    ts._ring[:n, 0] = d[:, None]
    ts._ring[:n, 1] = 0.2 + 0.5 * d[:, None] / 0.4
    ts._ring[:n, 2] = 0.5
    lead._state[L.S_DIST] = 0.4
    lead._state[L.S_POS_X], lead._state[L.S_POS_Y] = 0.7, 0.5
    env, _w = lead.Environment.device_tables(lead._device)
    out, diag = torch.empty((2, Bp), dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")

    def run(steps):
        for _ in range(steps):
            L.check(L.lib.riab_theta_sequence_step(env, L.ptr(lead._state), Bp, a.agents, L.ptr(ts._ring), n, n, 4 * n - 1, L.THETA_BEHIND,
                                                   0.3, float(ts.d_half), float(ts.theta_frac), None, None, 0, L.ptr(out),
                                                   L.ptr(diag), L.current_stream()), "riab_theta_sequence_step")

    run(20)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(1)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(g):
        run(a.steps)
    g.replay()
    torch.cuda.synchronize()
    us = events(g.replay, a.repeats, a.steps)
    return us, dict(lookback=n, finite=bool(torch.isfinite(out).all()), diag=diag.cpu().tolist())


def rollout_kernel(a):
    lead, ts, _pcs = build(a, True, False)
    for _ in range(30):
        lead.update()
    env, _w = lead.Environment.device_tables(lead._device)
    ts._rollout(ts._lead_state(), env, L.current_stream(), {})
    torch.cuda.synchronize()
    n = 10
    us = events(lambda: [ts._rollout(ts._lead_state(), env, L.current_stream(), {}) for _ in range(n)], a.repeats, n)
    count = ts.future_table[1][:a.agents].cpu().numpy()
    return us, dict(K=ts.rollout_steps_max, steps_min=int(count.min()), steps_mean=round(float(count.mean()), 1),
                    steps_max=int(count.max()), **ts.theta_diagnostics)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    runs = [("loop with sweep: Lead.update(); TS.update(); PCs(TS).update()", lambda: loop(a, True)),
            ("loop without: Lead.update(); PCs(Lead).update(), eager", lambda: loop(a, False, auto=False)),
            ("loop without: Lead.update(); PCs(Lead).update(), automatic step plan", lambda: loop(a, False, auto=True)),
            ("step kernel, look-behind, lookback 390", lambda: step_kernel(a, 390)),
            ("step kernel, look-behind, lookback 3906", lambda: step_kernel(a, 3906)),
            ("rollout kernel (us per rollout)", lambda: rollout_kernel(a))]
    lines = []
    for what, fn in runs:
        us, info = fn()
        med = statistics.median(us)
        lines.append(json.dumps(dict({"what": what, "agents": a.agents, "cells": a.cells, "steps": a.steps, "repeats": a.repeats,
                                      "us_median": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)},
                                     **info)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
