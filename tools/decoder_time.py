#!/usr/bin/env python
"""Time the linear decoder (csrc/riab_decoder.hip, ratinabox_amd/_decoder.py) on a long recorded run, beside the host
route it replaces and the measured float64 matrix-core ceiling: 4096 agents x 1024 PlaceCells x 256 recorded steps,
about 10^6 samples, m = 1027.

    hipcc --offload-arch=gfx950 -O3 tools/mfma_bench.hip -o tools/mfma_bench
    python tools/decoder_time.py [--agents 4096] [--cells 1024] [--steps 256] [--calls 4] [--repeats 5]
                                 [--host-steps 256] [--out profiles/decoder_time.txt]

The run is recorded by `--calls` simulate() calls, so the history spans that many chunks.  Device figures are timed with
HIP events around the whole call after two warm-up calls; reported: the MEDIAN over the repeats, min and max beside it.
  ceiling      tools/mfma_bench f64 (a child process): the best rate of a register-only v_mfma_f64_16x16x4_f64 loop
  moments      history_moments_tensor([PCs]): every chunk through riab_history_moments (both kernels, workspace
               allocation included).  FLOP: useful = m (m + 1) N (the lower triangle, 2 per product); executed = the
               16 x 16 tiles on and below the diagonal that the kernel multiplies, whole (the padding of m to 16 and of
               Bp to the 64-sample slab included)
  solve        LinearDecoder.from_moments (torch.linalg, float64, on the device), host clock with a synchronise
  decode       decode_tensor() over the same rows (riab_feedforward)
  host route   what a user does today, on the 16 cores of the job: every chunk's rates and positions `.cpu()`, widened to
               float64, X^T X / X^T y / sums accumulated with NumPy, the same ridge solve; host clock, once, over
               `--host-steps` rows, with the largest difference between the two fits' predictions on a sample of rows
One JSON line per figure."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ratinabox_amd as riab  # noqa: E402


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


def ceiling(binary):
    """(best TFLOP/s, the tool's lines) of the float64 loops of tools/mfma_bench, or (None, []) when it is not built"""
    if not os.path.exists(binary):
        return None, []
    out = subprocess.run([binary, "f64"], capture_output=True, text=True, timeout=300, check=True).stdout.splitlines()
    rates = [float(m.group(1)) for m in (re.search(r"([0-9.]+) TFLOP/s", l) for l in out if l.startswith("f64")) if m]
    return (max(rates) if rates else None), out


def host_route(ag, pcs, rows, alpha):
    """float64 normal equations on the host from `.cpu()` copies of the first `rows` rows, chunk by chunk"""
    n, B = int(pcs.n), ag._B
    G, C, sx, sy, N = np.zeros((n, n)), np.zeros((n, 2)), np.zeros(n), np.zeros(2), 0
    t_copy = t_math = 0.0
    left = rows
    for ca, cp, fa in zip(ag._hist.chunks, pcs._hist_fr.chunks, ag._hist.filled):   # (recorded together: same chunking)
        k = min(fa, left)
        if k <= 0:
            break
        left -= k
        t0 = time.perf_counter()
        x32 = cp[:k, :, :B].cpu().numpy()
        y32 = ca[:k, :2, :B].cpu().numpy()
        t1 = time.perf_counter()
        x = x32.transpose(0, 2, 1).reshape(-1, n).astype(np.float64)
        y = y32.transpose(0, 2, 1).reshape(-1, 2).astype(np.float64)
        G += x.T @ x
        C += x.T @ y
        sx += x.sum(axis=0)
        sy += y.sum(axis=0)
        N += len(x)
        t2 = time.perf_counter()
        t_copy += t1 - t0
        t_math += t2 - t1
    t0 = time.perf_counter()
    xbar, ybar = sx / N, sy / N
    W = np.linalg.solve(G - N * np.outer(xbar, xbar) + alpha * np.eye(n), C - N * np.outer(xbar, ybar))
    t_solve = time.perf_counter() - t0
    return W.T, ybar - xbar @ W, N, t_copy, t_math, t_solve


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.01)
    ap.add_argument("--host-steps", type=int, default=256)
    ap.add_argument("--mfma-bench", default=os.path.join(ROOT, "tools", "mfma_bench"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def report(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    peak, tool_lines = ceiling(a.mfma_bench)          # (before this process opens the device: one at a time)
    report(what="ceiling", f64_mfma_TFLOPs=peak, tool=[l for l in tool_lines if l.startswith("f64")] or "tools/mfma_bench not built")

    ag, pcs = record(a.agents, a.cells, a.steps, a.calls)
    rows = len(pcs._hist_fr)
    m = a.cells + 3
    N = rows * a.agents
    tiles = (lambda nt: nt * (nt + 1) // 2)((m + 15) // 16)            # the 16 x 16 tiles on and below the diagonal
    useful, executed = m * (m + 1) * N, tiles * 16 * 16 * 2 * rows * ((ag._Bp + 63) // 64 * 64)
    common = dict(agents=a.agents, cells=a.cells, rows=rows, chunks=len(pcs._hist_fr.chunks), m=m, samples=N, repeats=a.repeats)

    M, layout = riab.history_moments_tensor([pcs])
    ms = events(lambda: riab.history_moments_tensor([pcs]), a.repeats)
    med = statistics.median(ms)
    report(what="moments", ms_median=round(med, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
           useful_TFLOPs=round(useful / med * 1e-9, 2), executed_TFLOPs=round(executed / med * 1e-9, 2),
           useful_fraction_of_ceiling=None if not peak else round(useful / med * 1e-9 / peak, 3),
           executed_fraction_of_ceiling=None if not peak else round(executed / med * 1e-9 / peak, 3),
           rate_bytes=4 * a.cells * ag._Bp * rows, **common)

    def solve():
        t0 = time.perf_counter()
        d = riab.LinearDecoder.from_moments(M, layout, a.alpha)
        torch.cuda.synchronize()
        return d, time.perf_counter() - t0
    solve()
    ts = [solve()[1] for _ in range(a.repeats)]
    dec = solve()[0]
    report(what="solve", ms_median=round(1e3 * statistics.median(ts), 3), ms_min=round(1e3 * min(ts), 3),
           ms_max=round(1e3 * max(ts), 3), n_samples=dec.n_samples, n_dropped=dec.n_dropped, **common)

    ms = events(lambda: dec.decode_tensor(), a.repeats)
    med = statistics.median(ms)
    report(what="decode", ms_median=round(med, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
           TB_per_s_of_rates=round(4 * a.cells * ag._Bp * rows / med * 1e-9, 3),
           mean_error_m=float(dec.error().mean()), **common)

    hrows = min(a.host_steps, rows)
    coef, icpt, hN, t_copy, t_math, t_solve = host_route(ag, pcs, hrows, a.alpha)
    figures = dict(what="host route", rows=hrows, samples=hN, copy_s=round(t_copy, 3), normal_equations_s=round(t_math, 3),
                   solve_s=round(t_solve, 3), total_s=round(t_copy + t_math + t_solve, 3), threads=torch.get_num_threads())
    if hrows == rows:   # the same fit: how far apart the two decoders' predictions are
        x = pcs._hist_fr.chunks[0][:4, :, :64].permute(0, 2, 1).reshape(-1, a.cells).to(torch.float64)
        p_dev = (x @ dec.coef_.T + dec.intercept_).cpu().numpy()
        p_host = x.cpu().numpy() @ coef.T + icpt
        figures["max_prediction_difference_m"] = float(np.abs(p_dev - p_host).max())
    report(**figures)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
