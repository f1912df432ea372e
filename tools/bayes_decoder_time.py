#!/usr/bin/env python
"""Time the Bayesian decoder (csrc/riab_bayes.hip, ratinabox_amd/_bayes_decoder.py) on a recorded run, beside the feed-forward
kernel whose main loop it shares and the torch route it replaces: 4096 agents x 16 windows (65 536 samples) of 1024 and of 64
PlaceCells with spikes, against J = 400 and J = 4096 position bins — 2 n J M FLOP in the cross term, J M exponentials.

    python tools/bayes_decoder_time.py [--agents 4096] [--cells 1024,64] [--windows 16] [--window 5] [--bins 400,4096]
                                       [--repeats 10] [--out profiles/bayes_decoder_time.txt]

The grid is the environment's own (tuning="groundtruth", Environment.dx = 1 / sqrt(J)), so that J is exactly what is asked
for.  Device figures are timed with HIP events around the whole call after a warm-up call; reported: the MEDIAN over the
repeats, min and max beside it.  Per (J, population size):
  fit            fit_bayesian_decoder([pop], tuning="groundtruth") and (tuning="history", bins of the same size: the rate
                 maps of every recorded row, J as the edges make it): host clock with a synchronise
  decode         decode_all_tensor() over every recorded row: the window counts across the chunks, then the kernel
  kernel         riab_bayes_decode alone on the counts of the 16 windows into a preallocated tensor; FLOP = 2 n Jp M for the
                 cross term (Jp = J rounded up to 32: what the kernel multiplies), exponentials = Jp M
  ff yardstick   riab_feedforward n -> Jp outputs on 16 rate rows: the same main loop with a store epilogue, which writes
                 the (samples x Jp) matrix the decoder never does
  torch          the same mathematics with torch on the device: float32 matmul, log_softmax, argmax and the weighted mean,
                 which materialises (samples x J); and the largest difference of its posterior mean from the kernel's
One JSON line per figure."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ratinabox_amd as riab  # noqa: E402
from ratinabox_amd import _lib as L  # noqa: E402


def events(fn, repeats):
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


def spread(ms):
    return dict(ms_median=round(statistics.median(ms), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3))


def clocked(fn, repeats):
    def once():
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, 1e3 * (time.perf_counter() - t0)
    once()
    ts = [once()[1] for _ in range(repeats)]
    return once()[0], ts


def torch_route(counts, Lt, bias, centres):
    """counts (T, n, B) uint8 -> (posterior mean (T, 2, B), MAP bin (T, B)): the whole (T, J, B) log posterior in memory"""
    ell = torch.matmul(Lt, counts.to(torch.float32)) + bias[None, :, None]
    p = torch.log_softmax(ell, dim=1).exp_()
    return torch.matmul(centres, p), ell.argmax(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--cells", default="1024,64")
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--bins", default="400,4096")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def report(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    W = a.window
    for J in (int(j) for j in a.bins.split(",")):
        side = int(round(math.sqrt(J)))
        if side * side != J:
            raise SystemExit(f"--bins takes squares (the unit room's grid is side x side), got {J}")
        np.random.seed(1)
        env = riab.Environment({"dx": 1.0 / side})
        ag = riab.Agent(env, {"n_agents": a.agents, "dt": 0.05, "seed": 3})
        pops = [riab.PlaceCells(ag, {"n": int(c), "widths": 0.15, "max_fr": 10.0, "wall_geometry": "euclidean",
                                     "save_spikes": True, "name": f"PlaceCells{c}"}) for c in a.cells.split(",")]
        ag.simulate(a.windows * W)
        torch.cuda.synchronize()
        for pop in pops:
            n, rows_all = int(pop.n), len(pop._hist_sp)
            M = (rows_all // W) * ag._Bp
            common = dict(agents=a.agents, cells=n, bins=J, window=W, windows=rows_all // W, samples=M, repeats=a.repeats)
            dec, ts = clocked(lambda: riab.fit_bayesian_decoder([pop], tuning="groundtruth", window=W), a.repeats)
            assert dec.n_bins == J, (dec.n_bins, J)
            report(what="fit groundtruth", ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3),
                   ms_max=round(max(ts), 3), **common)
            try:
                hdec, ts = clocked(lambda: riab.fit_bayesian_decoder([pop], tuning="history", bin_size=1.0 / side, window=W,
                                                                     spikes=True), a.repeats)
                report(what="fit history (spikes)", ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3),
                       ms_max=round(max(ts), 3), bins_of_the_edges=hdec.n_bins, **common)
            except ValueError as e:
                report(what="fit history (spikes)", skipped=str(e), **common)

            ms = events(lambda: dec.decode_all_tensor(), a.repeats)
            report(what="decode", **spread(ms), chunks=len(pop._hist_sp.chunks), mean_error_m=float(dec.error().mean()), **common)

            dev = ag._device
            T, B, Jp = rows_all // W, ag._Bp, int(dec.S.shape[0])
            counts = torch.zeros((T, n, B), dtype=torch.uint8, device=dev)
            base = 0
            for chunk, filled in zip(pop._hist_sp.chunks, pop._hist_sp.filled):
                torch.ops.riab.history_window_counts(chunk[:filled], base, W, counts)
                base += filled
            bias = dec.bias(W)
            out = torch.empty((T, L.BAYES_OUT_ROWS, B), dtype=torch.float32, device=dev)
            arr = (L.RiabFFInput * 1)()
            arr[0].rates, arr[0].wt, arr[0].n_in = counts.data_ptr(), dec.log_rates[0].data_ptr(), n
            ms = events(lambda: L.check(L.lib.riab_bayes_decode(arr, 1, 1, 0.0, L.ptr(bias), L.ptr(dec.centres), J, Jp, T, B,
                                                                L.ptr(out), 0, L.current_stream()), "riab_bayes_decode"), a.repeats)
            med = statistics.median(ms)
            flop = 2.0 * n * Jp * T * B
            report(what="kernel", **spread(ms), cross_term_TFLOPs=round(flop / med * 1e-9, 2),
                   G_exponentials_per_s=round(Jp * T * B / med * 1e-6, 2), bins_padded=Jp, **common)

            rates = pop._hist_fr.chunks[0][:T]
            if int(rates.shape[0]) == T:
                zero = torch.zeros(Jp, dtype=torch.float32, device=dev)
                ms_ff = events(lambda: torch.ops.riab.feedforward([rates], dec.log_rates, zero, L.ACTIVATIONS["linear"], [0.0] * 4),
                               a.repeats)
                report(what="ff yardstick", **spread(ms_ff), TFLOPs=round(flop / statistics.median(ms_ff) * 1e-9, 2), n_out=Jp,
                       output_bytes=4 * Jp * T * B, kernel_over_ff=round(med / statistics.median(ms_ff), 3), **common)
            else:
                report(what="ff yardstick", skipped="the first chunk holds fewer rows than windows", **common)

            Lt = dec.log_rates[0][:, :J].T.contiguous()
            b32, c32 = bias[:J].contiguous(), dec.centres[:, :J].contiguous()
            ms_t = events(lambda: torch_route(counts, Lt, b32, c32), a.repeats)
            mean_t, arg_t = torch_route(counts, Lt, b32, c32)
            diff = float((mean_t[:, :, :ag._B] - out[:, 0:2, :ag._B]).abs().max())
            same = float((c32[0][arg_t[:, :ag._B]] == out[:, 2, :ag._B]).float().mean())
            report(what="torch", **spread(ms_t), kernel_over_torch=round(med / statistics.median(ms_t), 3),
                   max_mean_difference_from_kernel_m=diff, share_of_equal_MAP_x=same, intermediate_bytes=4 * J * T * B, **common)
            del counts, out, mean_t, arg_t
        del ag, pops
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
