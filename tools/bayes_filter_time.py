#!/usr/bin/env python
"""Time the Bayesian decoder's forward filter (csrc/riab_bayes_filter.hip, BayesianFilter in ratinabox_amd/_bayes_decoder.py) on
a recorded run, beside the memoryless decoder it extends and a torch route on the device: 4096 agents x 16 windows of 1024
and of 64 PlaceCells with spikes, against J = 400 and J = 4096 position bins.

    python tools/bayes_filter_time.py [--agents 4096] [--cells 1024,64] [--windows 16] [--window 5] [--bins 400,4096]
                                      [--repeats 10] [--out profiles/bayes_filter_time.txt]

The grid is the environment's own (tuning="groundtruth", Environment.dx = 1 / sqrt(J)).  Device figures are timed with HIP
events around the whole call after a warm-up call; reported: the MEDIAN over the repeats, min and max beside it.  Per (J,
population size):
  filter         BayesianFilter.decode_all_tensor(): the window counts, then per batch of windows riab_feedforward (the
                 likelihood stage, which writes windows x Jp x Bp float32) and riab_bayes_filter (the scan)
  scan           riab_bayes_filter alone on the log likelihood of the 16 windows (2 launches per window), per window; the
                 traffic a window cannot avoid is five [Jp][Bp] float32 passes (read the log likelihood; write l; read l; write
                 the x-blur; read it for the y-blur): achieved bytes/s = 5 x 4 Jp Bp / time per window
  memoryless     BayesianDecoder.decode_all_tensor() of the same windows (riab_bayes_decode: nothing of size J reaches memory)
  torch          the same recursion with torch on the device: float32 matmul for the likelihood of every window, then per
                 window log_softmax, exp and conv2d on the posterior reshaped to (Bp, 1, ny, nx); and the largest difference of
                 its posterior mean from the filter's
One JSON line per figure."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ratinabox_amd as riab  # noqa: E402
from ratinabox_amd import _lib as L  # noqa: E402
from ratinabox_amd import ops  # noqa: E402


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


def torch_route(counts, Lt, bias, filt, J):
    """counts (T, n, Bp) uint8 -> posterior mean (T, Bp, 2): the whole (T, Bp, J) log likelihood and, per window, the
    (Bp, J) posterior in memory"""
    ny, nx = filt.grid_shape
    R, eps = filt.radius, filt.mixing
    g = torch.tensor(filt.taps, dtype=torch.float32, device=counts.device)
    kern = torch.outer(g, g).reshape(1, 1, 2 * R + 1, 2 * R + 1)
    prior, inv = filt.prior[:J], filt.inv_norm[:J]
    ok = (inv > 0).to(torch.float32)
    centres = filt.decoder.centres[:, :J].T.contiguous()
    lik = torch.matmul(counts.to(torch.float32).permute(0, 2, 1), Lt) + bias[None, None, :]        # (T, Bp, J)
    logpred = torch.log(prior)[None, :]
    means = []
    for t in range(int(lik.shape[0])):
        p = torch.log_softmax(lik[t] + logpred, dim=1).exp_()
        means.append(p @ centres)
        q = (p * inv).reshape(-1, 1, ny, nx)
        pred = (1.0 - eps) * ok * torch.nn.functional.conv2d(q, kern, padding=R).reshape(-1, J) + eps * prior
        logpred = torch.log(pred)
    return torch.stack(means)


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
    if not torch.cuda.is_available():
        raise SystemExit("bayes_filter_time.py times the device: no GPU found")
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
            T, B = rows_all // W, ag._Bp
            dec = riab.fit_bayesian_decoder([pop], tuning="groundtruth", window=W)
            assert dec.n_bins == J, (dec.n_bins, J)
            filt = dec.with_continuity()
            Jp = int(dec.S.shape[0])
            common = dict(agents=a.agents, cells=n, bins=J, bins_padded=Jp, window=W, windows=T, radius=filt.radius,
                          sigma_m=round(filt.sigma, 5), mixing=filt.mixing, repeats=a.repeats)
            ms_f = events(lambda: filt.decode_all_tensor(), a.repeats)
            report(what="filter", **spread(ms_f), mean_error_m=float(filt.error().mean()), **common)
            ms_m = events(lambda: dec.decode_all_tensor(), a.repeats)
            report(what="memoryless", **spread(ms_m), mean_error_m=float(dec.error().mean()),
                   filter_over_memoryless=round(statistics.median(ms_f) / statistics.median(ms_m), 3), **common)

            dev = ag._device
            counts = torch.zeros((T, n, B), dtype=torch.uint8, device=dev)
            base = 0
            for chunk, filled in zip(pop._hist_sp.chunks, pop._hist_sp.filled):
                torch.ops.riab.history_window_counts(chunk[:filled], base, W, counts)
                base += filled
            bias = filt._lik_bias(W)
            loglik = torch.ops.riab.feedforward([counts.to(torch.float32)], dec.log_rates, bias, L.ACTIVATIONS["linear"], [0.0] * 4)
            post, tmp = (torch.empty((Jp, B), dtype=torch.float32, device=dev) for _ in range(2))
            ws = torch.empty(ops.bayes_filter_workspace_floats(Jp, B), dtype=torch.float32, device=dev)
            out = torch.empty((T, L.BAYES_OUT_ROWS, B), dtype=torch.float32, device=dev)
            ny, nx = filt.grid_shape
            ms_s = events(lambda: torch.ops.riab.bayes_filter(loglik, J, ny, nx, filt._taps32, filt.mixing, filt.prior, filt.inv_norm,
                                                              dec.centres, None, True, post, tmp, ws, out), a.repeats)
            per_window = statistics.median(ms_s) / T
            floor_bytes = 5 * 4 * Jp * B
            report(what="scan", **spread(ms_s), ms_per_window=round(per_window, 4), launches=2 * T, bytes_per_window_floor=floor_bytes,
                   achieved_GBps_of_the_floor=round(floor_bytes / per_window * 1e-6, 1), scan_share_of_filter=round(
                       statistics.median(ms_s) / statistics.median(ms_f), 3), **common)
            mean_f = out[:, 0:2, :ag._B].permute(0, 2, 1)
            del loglik

            Lt = dec.log_rates[0][:, :J].contiguous()
            b32 = bias[:J].contiguous()
            try:
                ms_t = events(lambda: torch_route(counts, Lt, b32, filt, J), a.repeats)
                mean_t = torch_route(counts, Lt, b32, filt, J)[:, :ag._B]
                report(what="torch", **spread(ms_t), filter_over_torch=round(statistics.median(ms_f) / statistics.median(ms_t), 3),
                       max_mean_difference_from_filter_m=float((mean_t - mean_f).abs().max()), intermediate_bytes=4 * J * T * B, **common)
                del mean_t
            except RuntimeError as e:
                report(what="torch", failed=str(e).splitlines()[0][:200], **common)
            del counts, out, post, tmp, ws
        del ag, pops
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
