#!/usr/bin/env python
"""Time the Gaussian-process decoder (csrc/riab_gp.hip, ratinabox_amd/_gp_decoder.py) on a recorded run, beside the routes it
replaces and the feed-forward kernel whose main loop it shares: 4096 agents x 1024 PlaceCells, 16 recorded rows (65 536
queries) against N = 2048 training samples — 2 n N M = 2.7e11 FLOP in the cross term — and the same with a 64-cell
population, where the exponential and not the matrix cores sets the pace.

    python tools/gp_decoder_time.py [--agents 4096] [--cells 1024,64] [--steps 16] [--train 2048] [--repeats 10]
                                    [--host-queries 2048] [--out profiles/gp_decoder_time.txt]

Device figures are timed with HIP events around the whole call after a warm-up call; reported: the MEDIAN over the repeats,
min and max beside it.  Per population size:
  fit            fit_gp_decoder([pop], max_samples=N): the gather from the chunks, the Gram matrix, the Cholesky factor and
                 the solve (torch, float64, on the device); host clock with a synchronise.  `solve` is from_samples alone.
  decode         decode_tensor() over every recorded row (riab_gp_predict per chunk, output allocation included)
  kernel         riab_gp_predict alone on the first chunk's rows into a preallocated tensor; FLOP = 2 n Np M for the cross
                 term (Np = N rounded up to 32: what the kernel multiplies), exponentials = Np M
  ff yardstick   riab_feedforward n -> N outputs on the same rows: the same main loop with a store epilogue
  torch          the same mathematics with torch on the device, one row (B queries) at a time: matmul, exp, matmul in fp32,
                 which writes and re-reads a B x N matrix per row; and its largest difference from the kernel's output
  host route     what a user does today: the rates `.cpu()`, sklearn's GaussianProcessRegressor.predict on the cores of the
                 job for `--host-queries` queries, SCALED to all M (said so in the line)
One JSON line per figure."""
import argparse
import json
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


def torch_route(rows, Xt32, sq_t, alT, inv):
    """rows (T, n, B) fp32 -> (T, D, B): per row, cross = X (N, n) @ r (n, B), k = exp(-max(0, d2) inv), out = alpha^T @ k"""
    out = torch.empty((rows.shape[0], alT.shape[0], rows.shape[2]), dtype=torch.float32, device=rows.device)
    for t in range(rows.shape[0]):
        r = rows[t]
        d2 = (r * r).sum(dim=0)[None, :] + sq_t[:, None] - 2.0 * (Xt32 @ r)
        out[t] = alT @ torch.exp(d2.clamp_(min=0.0).mul_(-inv))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--cells", default="1024,64")
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--train", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-queries", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def report(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    np.random.seed(1)
    ag = riab.Agent(riab.Environment({}), {"n_agents": a.agents, "dt": 0.01, "seed": 3})
    pops = [riab.PlaceCells(ag, {"n": int(c), "widths": 0.2, "wall_geometry": "euclidean", "save_spikes": False,
                                 "name": f"PlaceCells{c}"}) for c in a.cells.split(",")]
    ag.simulate(a.steps)
    torch.cuda.synchronize()
    for pop in pops:
        n, rows_all = int(pop.n), len(pop._hist_fr)
        M = rows_all * ag._Bp
        common = dict(agents=a.agents, cells=n, rows=rows_all, queries=M, repeats=a.repeats)

        def fit():
            t0 = time.perf_counter()
            d = riab.fit_gp_decoder([pop], max_samples=a.train)
            torch.cuda.synchronize()
            return d, time.perf_counter() - t0
        fit()
        ts = [fit()[1] for _ in range(a.repeats)]
        dec = fit()[0]
        N, Np = dec.n_samples, (dec.n_samples + 31) // 32 * 32
        X, y = dec.X_train_, dec.alpha_.new_zeros(N, 2)

        def solve():
            t0 = time.perf_counter()
            riab.GPDecoder.from_samples(X, y + 1.0, dec.length_scale, dec.alpha)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        solve()
        ss = [solve() for _ in range(a.repeats)]
        report(what="fit", ms_median=round(1e3 * statistics.median(ts), 3), ms_min=round(1e3 * min(ts), 3),
               ms_max=round(1e3 * max(ts), 3), solve_ms_median=round(1e3 * statistics.median(ss), 3), n_train=N,
               n_dropped=dec.n_dropped, length_scale=dec.length_scale, **common)

        ms = events(lambda: dec.decode_tensor(), a.repeats)
        report(what="decode", **spread(ms), chunks=len(pop._hist_fr.chunks), mean_error_m=float(dec.error().mean()), **common)

        rows = pop._hist_fr.chunks[0][:pop._hist_fr.filled[0]]
        T, B = int(rows.shape[0]), int(rows.shape[2])
        wts, sq, al = dec._device_tables(rows.device)
        inv = 1.0 / (2.0 * dec.length_scale ** 2)
        out = torch.empty((T, 2, B), dtype=torch.float32, device=rows.device)
        arr = (L.RiabFFInput * 1)()
        arr[0].rates, arr[0].wt, arr[0].n_in = rows.data_ptr(), wts[0].data_ptr(), n
        ms = events(lambda: L.check(L.lib.riab_gp_predict(arr, 1, L.ptr(sq), L.ptr(al), 2, N, inv, T, B, L.ptr(out),
                                                          L.current_stream()), "riab_gp_predict"), a.repeats)
        med = statistics.median(ms)
        flop = 2.0 * n * Np * T * B
        report(what="kernel", **spread(ms), cross_term_TFLOPs=round(flop / med * 1e-9, 2),
               G_exponentials_per_s=round(Np * T * B / med * 1e-6, 2), rows_timed=T, n_train_padded=Np, **common)

        bias = torch.zeros(Np, dtype=torch.float32, device=rows.device)
        ms_ff = events(lambda: torch.ops.riab.feedforward([rows], wts, bias, L.ACTIVATIONS["linear"], [0.0] * 4), a.repeats)
        report(what="ff yardstick", **spread(ms_ff), TFLOPs=round(flop / statistics.median(ms_ff) * 1e-9, 2), n_out=Np,
               output_bytes=4 * Np * T * B, **common)

        Xt32, alT = X.to(torch.float32), al[:, :N].contiguous()
        ms_t = events(lambda: torch_route(rows, Xt32, sq[:N], alT, inv), a.repeats)
        diff = float((torch_route(rows, Xt32, sq[:N], alT, inv)[:, :, :ag._B] - out[:, :, :ag._B]).abs().max())
        report(what="torch", **spread(ms_t), kernel_over_torch=round(med / statistics.median(ms_t), 3),
               max_difference_from_kernel=diff, alpha_l1=[float(v) for v in dec.alpha_.abs().sum(dim=0)], **common)

        try:
            from sklearn.gaussian_process import GaussianProcessRegressor
            from sklearn.gaussian_process.kernels import RBF
        except ImportError:
            report(what="host route", skipped="scikit-learn is not installed", **common)
            continue
        q = min(a.host_queries, B)
        t0 = time.perf_counter()
        xq = rows[0, :, :q].cpu().numpy().T.astype(np.float64)
        t_copy = time.perf_counter() - t0
        gp = GaussianProcessRegressor(alpha=dec.alpha, kernel=RBF(dec.length_scale, length_scale_bounds="fixed"))
        t0 = time.perf_counter()
        gp.fit(X.cpu().numpy(), np.zeros((N, 2)) + 1.0)
        t_fit = time.perf_counter() - t0
        t0 = time.perf_counter()
        gp.predict(xq)
        t_pred = time.perf_counter() - t0
        report(what="host route", queries_timed=q, copy_s=round(t_copy, 4), sklearn_fit_s=round(t_fit, 3),
               predict_s=round(t_pred, 4), predict_s_SCALED_to_all_queries=round(t_pred * M / q, 2),
               copy_s_SCALED_to_all_queries=round(t_copy * M / q, 3), threads=torch.get_num_threads(), **common)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
