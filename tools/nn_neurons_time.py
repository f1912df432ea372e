#!/usr/bin/env python
"""Time contribs.NeuralNetworkNeurons against what the package offered before it — the same network as three chained
FeedForwardLayers — on the same build, in one process: 4096 agents x 1024 PlaceCells into the default MLP shape
(1024 -> 20 -> 20 -> 16, relu, relu, linear).

    python tools/nn_neurons_time.py [--agents 4096] [--cells 1024] [--steps 1024] [--loop-steps 200] [--repeats 7]
                                    [--warmup 2] [--out profiles/nn_neurons_time.txt]

Two regimes, three variants in each:
  loop      `Ag.update(); PCs.update(); N.update()` per step (the chain: `...; F1.update(); F2.update(); F3.update()`),
            `--loop-steps` steps per repeat
  simulate  `Ag.simulate(--steps)`
  variants  engine="auto" (the fused kernel, riab_mlp_forward), engine="torch" (the module itself on the device), and the
            chain of FeedForwardLayers — the BASELINE every ratio is taken against.

Method: the device is synchronised before and after a timed region and the region is timed on the host
clock (the loop regime is bound by the host's launches; a simulate() call returns while its kernels run), the variants take
turns repeat by repeat so that a drift of the clocks lands on all of them, the first `--warmup` repeats are dropped, and the
figure reported is the MEDIAN over the repeats with min and max beside it.  Nobody keeps a history or draws spikes (rows are
overwritten in place / in a ring).  The engine that served each variant is recorded: the chain's unchanged per-step loop
is taken over by a native step plan (plan.AutoStepper) and its simulate() is one native call, while a NeuralNetworkNeurons
population cannot be held by a step plan yet, so its loop stays eager and its simulate() is the chunk engine.
No threshold is applied: the last lines give the ratios to the chain with their run-to-run range."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ratinabox_amd as riab  # noqa: E402
from ratinabox_amd.contribs.NeuralNetworkNeurons import NeuralNetworkNeurons, MultiLayerPerceptron  # noqa: E402

QUIET = {"save_history": False, "save_spikes": False}
VARIANTS = ("fused", "torch", "ff_chain")


def make(variant, agents, cells):
    np.random.seed(1)
    torch.manual_seed(1)
    ag = riab.Agent(riab.Environment({}), {"n_agents": agents, "dt": 0.01, "seed": 3, "save_history": False})
    pcs = riab.PlaceCells(ag, dict(QUIET, n=cells, name="PCs"))
    if variant == "ff_chain":
        pops, prev = [pcs], pcs
        for i, (n, act) in enumerate(((20, "relu"), (20, "relu"), (16, "linear"))):
            prev = riab.FeedForwardLayer(ag, dict(QUIET, n=n, input_layers=[prev], name=f"F{i}",
                                                  activation_function={"activation": act}))
            pops.append(prev)
        return ag, pops
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        N = NeuralNetworkNeurons(ag, dict(QUIET, input_layers=[pcs], NeuralNetworkModule=MultiLayerPerceptron(cells, 16, [20, 20]),
                                          engine="auto" if variant == "fused" else "torch"))
    assert N.engine == variant
    return ag, [pcs, N]


def time_loop(ag, pops, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ag.update()
        for p in pops:
            p.update()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def time_simulate(ag, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ag.simulate(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--loop-steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5, "at least 5 repeats each"
    lines = []
    for regime in ("loop", "simulate"):
        worlds = {v: make(v, a.agents, a.cells) for v in VARIANTS}     # (fresh worlds per regime: a loop's plan is not carried over)
        us = {v: [] for v in VARIANTS}
        served = {}
        for r in range(a.warmup + a.repeats):
            for v in VARIANTS:                                          # alternating
                ag, pops = worlds[v]
                before = dict(ag.engine_runs)
                t = time_loop(ag, pops, a.loop_steps) if regime == "loop" else time_simulate(ag, a.steps)
                if r >= a.warmup:
                    us[v].append(t)
                    if regime == "loop":
                        served[v] = type(ag._plan).__name__ if ag._plan is not None else "eager"
                    else:
                        served[v] = "+".join(k for k in ag.engine_runs if ag.engine_runs[k] != before[k])
        for v in VARIANTS:
            med = statistics.median(us[v])
            lines.append(json.dumps({"regime": regime, "variant": v, "agents": a.agents, "cells": a.cells,
                                     "steps": a.loop_steps if regime == "loop" else a.steps, "warmup": a.warmup,
                                     "repeats": a.repeats, "us_per_step_median": round(med, 3), "us_min": round(min(us[v]), 3),
                                     "us_max": round(max(us[v]), 3), "served_by": served[v]}))
            print(lines[-1], flush=True)
        base = us["ff_chain"]
        for v in ("fused", "torch"):
            lines.append(json.dumps({"regime": regime, "ratio": f"{v} / ff_chain (baseline)",
                                     "of_medians": round(statistics.median(us[v]) / statistics.median(base), 3),
                                     "lowest": round(min(us[v]) / max(base), 3), "highest": round(max(us[v]) / min(base), 3)}))
            print(lines[-1], flush=True)
        del worlds
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
