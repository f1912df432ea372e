#!/usr/bin/env python
"""Time one TD learning step of contribs.ValueNeuron's kernels (csrc/riab_td.hip) against the same step written with
stock PyTorch on the same card, at the flagship batch: 4096 agents x 1024 input cells, n = 1 (ValueNeuron) and n = 64
(SuccessorFeatures over 64 features).

    python tools/td_time.py [--steps 200] [--repeats 7] [--agents 4096] [--cells 1024]

What is timed (HIP events around `steps` back-to-back steps after a warm-up; the figure of a repeat is its mean per
step, the figure reported is the MEDIAN over the repeats, min and max beside it; each variant is timed twice, as eager
calls from Python and as one captured graph of `steps` steps, which leaves the device's time alone):
  hip_fused    torch.ops.riab.td_update(fuse_trace=True): trace update + TD error + batch gradient in one kernel, the
               fixed-order combine and weight update in a second
  hip_plain    torch.ops.riab.td_forward_tail(with_trace=True) + td_update(fuse_trace=False): the trace is read twice
  torch        e.mul_(k).add_(phi, alpha=dt); g = (r + dVdt - V / tau) * prime; G = g[:, :B] @ e[:, :B].T;
               W.mul_(1 - decay).add_(G, alpha=scale)
Every variant prints one JSON line; bytes = the algorithmic traffic of the fused form (12 n_in B for phi and the
trace, 12 n B for V, dV/dt and prime + 4 n B for the TD error + the weights' and partial sums' traffic)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ratinabox_amd  # noqa: F401,E402
from ratinabox_amd import ops  # noqa: F401,E402


def timed(fn, steps, repeats, warmup=20, graph=False):
    """us per step of each repeat.  graph: the `steps` steps are captured once in a torch.cuda.graph and a repeat is one
    replay — the device's time without the host's per-call work (both sides profit alike)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    if graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(steps):
                fn()
        g.replay()
        torch.cuda.synchronize()
        out = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) * 1e3 / steps)
        return out
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--cells", type=int, default=1024)
    a = ap.parse_args()
    dev = torch.device("cuda")
    B = Bp = a.agents
    n_in = a.cells
    dt, tau, tau_e, eta, L2 = 0.05, 1.0, 0.25, 0.001, 0.001
    consts = [dt, tau, tau_e, eta, L2]
    for n in (1, 64):
        Mp = (n + 31) // 32 * 32
        g = torch.Generator(device="cpu").manual_seed(n)
        phi = torch.rand((n_in, Bp), generator=g).to(dev)
        trace = torch.zeros((n_in, Bp), device=dev)
        wt = (torch.randn((n_in, Mp), generator=g) * 0.03).to(dev)
        wt[:, n:] = 0
        v, v_last, dvdt = (torch.rand((n, Bp), generator=g).to(dev) for _ in range(3))
        prime = torch.ones((n, Bp), device=dev)
        td = torch.zeros((n, Bp), device=dev)
        rew = torch.rand((n, Bp), generator=g).to(dev)
        floats = ops.td_workspace_floats(n, [n_in], Bp)
        ws = torch.empty(floats, dtype=torch.float32, device=dev)
        w_plain = wt[:, :n].t().contiguous()
        k_e, scale, decay = 1.0 - dt / tau_e, dt * eta / B, eta * dt * L2

        def hip_fused():
            torch.ops.riab.td_update([wt], [trace], [phi], rew, v, dvdt, prime, td, ws, consts, B, True)

        def hip_plain():
            torch.ops.riab.td_forward_tail(v, v_last, dvdt, [phi], [trace], [wt], consts, B, True)
            torch.ops.riab.td_update([wt], [trace], [phi], rew, v, dvdt, prime, td, ws, consts, B, False)

        def stock():
            trace.mul_(k_e).add_(phi, alpha=dt)
            gg = (rew + dvdt - v / tau) * prime
            G = gg[:, :B] @ trace[:, :B].t()
            w_plain.mul_(1.0 - decay).add_(G, alpha=scale)

        nbytes = 12 * n_in * B + 16 * n * B + 2 * 4 * floats + 2 * 4 * n * n_in
        flop = 2 * Mp * n_in * B
        for name, fn, graph in [(k, f, m) for m in (False, True) for k, f in (("hip_fused", hip_fused), ("hip_plain", hip_plain),
                                                                               ("torch", stock))]:
            us = timed(fn, a.steps, a.repeats, graph=graph)
            med = statistics.median(us)
            print(json.dumps({"variant": name, "mode": "graph replay" if graph else "eager calls", "n": n, "agents": B, "cells": n_in, "steps": a.steps, "repeats": a.repeats,
                              "us_per_step_median": round(med, 3), "us_min": round(min(us), 3), "us_max": round(max(us), 3),
                              "fused_bytes": nbytes, "mfma_flop": flop,
                              "TB_per_s_of_fused_bytes": round(nbytes / med * 1e-6, 3),
                              "fraction_of_8TBps": round(nbytes / med * 1e-6 / 8.0, 3)}), flush=True)


if __name__ == "__main__":
    main()
