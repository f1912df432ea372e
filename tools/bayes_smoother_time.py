#!/usr/bin/env python
"""Time the Bayesian decoder's backward smoother (csrc/riab_bayes_smooth.hip, BayesianSmoother in
ratinabox_amd/_bayes_decoder.py) on a recorded run, in the same run as the forward filter it stands behind and a torch route on
the device: 4096 agents x 16 windows of 1024 and of 64 PlaceCells with spikes, against J = 400 and J = 4096 position bins
(the four columns of tools/bayes_filter_time.py, whose set-up and timing method this keeps).

    python tools/bayes_smoother_time.py [--agents 4096] [--cells 1024,64] [--windows 16] [--window 5] [--bins 400,4096]
                                        [--repeats 10] [--out profiles/bayes_smoother_time.txt]

Device figures are timed with HIP events around the whole call after a warm-up call; reported: the MEDIAN over the repeats, min
and max beside it.  Per (J, population size):
  smoother       BayesianSmoother.decode_all_tensor(): the window counts, riab_feedforward (the likelihood), the forward scan
                 with l kept (riab_bayes_filter_keep), the backward scan (riab_bayes_smooth)
  filter         BayesianFilter.decode_all_tensor() of the same windows
  forward scan   riab_bayes_filter alone on the log likelihood of the 16 windows, per window (what tools/bayes_filter_time.py
                 reports as "scan"); forward scan kept: riab_bayes_filter_keep, the same
  backward scan  riab_bayes_smooth alone, per window, and its ratio to the forward scan.  It moves six [Jp][Bp] float32 passes
                 a window cannot avoid (read l and tmp's taps, write beta; read the log likelihood and beta, write tmp)
                 against the forward scan's five
  torch          forward-backward with torch on the device: float32 matmul for the likelihood, then per window log_softmax,
                 exp and conv2d forwards, and exp and conv2d backwards on the (Bp, J) arrays; and the largest difference of
                 its smoothed posterior mean from the smoother's
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ratinabox_amd as riab  # noqa: E402
from bayes_filter_time import events, spread  # noqa: E402
from ratinabox_amd import _lib as L  # noqa: E402
from ratinabox_amd import ops  # noqa: E402


def torch_route(counts, Lt, bias, filt, J):
    """counts (T, n, Bp) uint8 -> smoothed posterior mean (T, Bp, 2): the (T, Bp, J) log likelihood and posteriors in memory"""
    ny, nx = filt.grid_shape
    R, eps = filt.radius, filt.mixing
    g = torch.tensor(filt.taps, dtype=torch.float32, device=counts.device)
    kern = torch.outer(g, g).reshape(1, 1, 2 * R + 1, 2 * R + 1)
    prior, inv = filt.prior[:J], filt.inv_norm[:J]
    ok = (inv > 0).to(torch.float32)
    centres = filt.decoder.centres[:, :J].T.contiguous()
    lik = torch.matmul(counts.to(torch.float32).permute(0, 2, 1), Lt) + bias[None, None, :]        # (T, Bp, J)
    T = int(lik.shape[0])
    logpred = torch.log(prior)[None, :]
    post, ratio = [], []                                      # p_t and p_t / pred_t = exp(loglik_t - ev_t)
    for t in range(T):
        ell = lik[t] + logpred
        ev = torch.logsumexp(ell, dim=1, keepdim=True)
        p = (ell - ev).exp_()
        post.append(p)
        ratio.append((lik[t] - ev).exp_())
        q = (p * inv).reshape(-1, 1, ny, nx)
        pred = (1.0 - eps) * ok * torch.nn.functional.conv2d(q, kern, padding=R).reshape(-1, J) + eps * prior
        logpred = torch.log(pred)
    means = [None] * T
    means[T - 1] = post[T - 1] @ centres
    beta = None
    for t in range(T - 2, -1, -1):
        u = ratio[t + 1] if beta is None else ratio[t + 1] * beta
        c = u @ prior
        beta = (1.0 - eps) * inv * torch.nn.functional.conv2d(u.reshape(-1, 1, ny, nx), kern, padding=R).reshape(-1, J) \
            + eps * c[:, None] * ok
        gm = post[t] * beta
        means[t] = (gm @ centres) / gm.sum(dim=1, keepdim=True)
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
        raise SystemExit("bayes_smoother_time.py times the device: no GPU found")
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
            sm = filt.smoothed()
            Jp = int(dec.S.shape[0])
            keeps, blocks = sm.column_blocks(T, B)
            common = dict(agents=a.agents, cells=n, bins=J, bins_padded=Jp, window=W, windows=T, radius=filt.radius,
                          sigma_m=round(filt.sigma, 5), mixing=filt.mixing, repeats=a.repeats)
            ms_sm = events(lambda: sm.decode_all_tensor(), a.repeats)
            ms_f = events(lambda: filt.decode_all_tensor(), a.repeats)
            report(what="smoother", **spread(ms_sm), mean_error_m=float(sm.error().mean()), likelihood_kept=keeps,
                   column_blocks=len(blocks), smoother_over_filter=round(statistics.median(ms_sm) / statistics.median(ms_f), 3), **common)
            report(what="filter", **spread(ms_f), mean_error_m=float(filt.error().mean()),
                   memoryless_mean_error_m=float(dec.error().mean()), **common)

            dev = ag._device
            counts = torch.zeros((T, n, B), dtype=torch.uint8, device=dev)
            base = 0
            for chunk, filled in zip(pop._hist_sp.chunks, pop._hist_sp.filled):
                torch.ops.riab.history_window_counts(chunk[:filled], base, W, counts)
                base += filled
            bias = filt._lik_bias(W)
            loglik = torch.ops.riab.feedforward([counts.to(torch.float32)], dec.log_rates, bias, L.ACTIVATIONS["linear"], [0.0] * 4)
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
            post, tmp, ws, out = new(Jp, B), new(Jp, B), new(ops.bayes_filter_workspace_floats(Jp, B)), new(T, L.BAYES_OUT_ROWS, B)
            ny, nx = filt.grid_shape
            tables = (filt._taps32, filt.mixing, filt.prior, filt.inv_norm, dec.centres)
            ms_s = events(lambda: torch.ops.riab.bayes_filter(loglik, J, ny, nx, *tables, None, True, post, tmp, ws, out), a.repeats)
            fwd = statistics.median(ms_s) / T
            report(what="forward scan", **spread(ms_s), ms_per_window=round(fwd, 4), launches=2 * T,
                   bytes_per_window_floor=5 * 4 * Jp * B, achieved_GBps_of_the_floor=round(5 * 4 * Jp * B / fwd * 1e-6, 1), **common)
            ells, filtered = new(T, Jp, B), new(T, L.BAYES_OUT_ROWS, B)
            ms_k = events(lambda: torch.ops.riab.bayes_filter_keep(loglik, J, ny, nx, *tables, None, True, ells, tmp, ws, filtered),
                          a.repeats)
            report(what="forward scan kept", **spread(ms_k), ms_per_window=round(statistics.median(ms_k) / T, 4), launches=2 * T,
                   same_bits_as_forward_scan=bool(torch.equal(filtered, out)), **common)
            beta, ws2 = new(Jp, B), new(ops.bayes_smooth_workspace_floats(Jp, B))
            ms_b = events(lambda: torch.ops.riab.bayes_smooth(loglik, ells, filtered, J, ny, nx, *tables, None, True, beta, tmp, ws2, out),
                          a.repeats)
            bwd = statistics.median(ms_b) / T
            report(what="backward scan", **spread(ms_b), ms_per_window=round(bwd, 4), launches=2 * T,
                   bytes_per_window_floor=6 * 4 * Jp * B, achieved_GBps_of_the_floor=round(6 * 4 * Jp * B / bwd * 1e-6, 1),
                   backward_over_forward=round(bwd / fwd, 3), backward_scan_share_of_smoother=round(
                       statistics.median(ms_b) / statistics.median(ms_sm), 3), **common)
            mean_s = out[:, 0:2, :ag._B].permute(0, 2, 1).clone()
            del loglik, ells

            Lt = dec.log_rates[0][:, :J].contiguous()
            b32 = bias[:J].contiguous()
            try:
                ms_t = events(lambda: torch_route(counts, Lt, b32, filt, J), a.repeats)
                mean_t = torch_route(counts, Lt, b32, filt, J)[:, :ag._B]
                report(what="torch", **spread(ms_t), smoother_over_torch=round(statistics.median(ms_sm) / statistics.median(ms_t), 3),
                       max_mean_difference_from_smoother_m=float((mean_t - mean_s).abs().max()), intermediate_bytes=3 * 4 * J * T * B,
                       **common)
                del mean_t
            except RuntimeError as e:
                report(what="torch", failed=str(e).splitlines()[0][:200], **common)
            del counts, out, post, tmp, ws, ws2, beta, filtered
        del ag, pops
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
