#!/usr/bin/env python
"""Time the Gaussian-process decoder's predictive variance (riab_gp_predict_var in csrc/riab_gp.hip,
GPDecoder.predict_tensor(return_std=True)) beside the mean-only call and a torch route on the device: 4096 agents x 16
recorded rows (65 536 queries) against N = 2048 training samples, with 1024 and with 64 PlaceCells.

    python tools/gp_variance_time.py [--agents 4096] [--cells 1024,64] [--steps 16] [--train 2048] [--repeats 10]
                                     [--out profiles/gp_variance_time.txt]

Device figures are timed with HIP events around the whole call after a warm-up call; reported: the MEDIAN over the repeats,
min and max beside it.  Per population size:
  table          GPDecoder._variance_table: K + alpha I factorised again in float64, L^-1 by a triangular solve against the
                 identity, transposed to float32 (once per decoder and device); host clock with a synchronise
  std            predict_tensor(rows, return_std=True) at the default max_workspace_bytes (the pieces are reported): both
                 stages of every piece, the output and workspace allocations and the square root
  abi            riab_gp_predict_var alone on as many rows as one default workspace holds, everything preallocated
  stages         the two kernels of that call apart, from torch.profiler's device times (mean over the profiled calls; the
                 profiler perturbs less than it resolves here, its sum is printed beside the event-timed call).
                 stage 2 FLOP = M Np^2 (the triangular half of 2 M Np^2; the kernel multiplies Np^2 (1 + 128 / Np) M of it,
                 whole 128-row blocks); stage 1 is the mean's kernel plus 4 Np M bytes of stores
  mean           riab_gp_predict through predict_tensor(rows) on the same rows
  torch          the same mathematics with torch on the device in float32, one row (B queries) at a time: kernel_matrix,
                 solve_triangular against the float32 factor, square, sum; and its largest difference from the kernel's var
  float64        the largest difference of the kernel's var from GPDecoder.std_float64 ** 2 on 256 queries
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
from ratinabox_amd._gp_decoder import workspace_pieces  # noqa: E402


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


def torch_route(rows, X32, sq_t, L32, inv):
    """rows (T, n, B) fp32 -> var (T, B): per row k* = exp(-max(0, d2) inv) (N, B), V = L^-1 k*, 1 - sum V^2, clamped"""
    out = torch.empty((rows.shape[0], rows.shape[2]), dtype=torch.float32, device=rows.device)
    for t in range(rows.shape[0]):
        r = rows[t]
        d2 = (r * r).sum(dim=0)[None, :] + sq_t[:, None] - 2.0 * (X32 @ r)
        V = torch.linalg.solve_triangular(L32, torch.exp(d2.clamp_(min=0.0).mul_(-inv)), upper=False)
        out[t] = (1.0 - (V * V).sum(dim=0)).clamp_(min=0.0)
    return out


def stage_times(fn, calls):
    """{kernel name fragment: mean device microseconds per call} of the GP kernels, from torch.profiler"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        us = getattr(e, "device_time_total", None)
        if us is None:
            us = getattr(e, "cuda_time_total", 0.0)
        for frag in ("gp_var_kernel", "gp_kernel"):
            if frag in e.key:
                out[frag] = out.get(frag, 0.0) + us / calls
                break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--cells", default="1024,64")
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--train", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def report(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    np.random.seed(1)
    ag = riab.Agent(riab.Environment({}), {"n_agents": a.agents, "dt": 0.01, "seed": 3})
    pops = [riab.PlaceCells(ag, {"n": int(c), "widths": 0.2, "wall_geometry": "euclidean", "save_spikes": False,
                                 "name": f"PlaceCells{c}"}) for c in a.cells.split(",")]
    ag.simulate(a.steps)
    torch.cuda.synchronize()
    for pop in pops:
        n = int(pop.n)
        rows = pop._hist_fr.chunks[0][:pop._hist_fr.filled[0]]
        T, B = int(rows.shape[0]), int(rows.shape[2])
        dec = riab.fit_gp_decoder([pop], max_samples=a.train)
        N, Np = dec.n_samples, (dec.n_samples + 31) // 32 * 32
        common = dict(agents=a.agents, cells=n, rows=T, queries=T * B, n_train=N, repeats=a.repeats)

        def table():
            dec._linv_t = None
            t0 = time.perf_counter()
            dec._variance_table(rows.device)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        table()
        ts = [table() for _ in range(3)]
        report(what="table", ms_median=round(1e3 * statistics.median(ts), 1), ms_min=round(1e3 * min(ts), 1),
               ms_max=round(1e3 * max(ts), 1), table_bytes=4 * Np * Np, length_scale=dec.length_scale,
               log_marginal_likelihood=dec.log_marginal_likelihood_, **common)

        pieces = workspace_pieces(T, B, Np, 2 ** 28)
        ms_std = events(lambda: dec.predict_tensor([rows], return_std=True), a.repeats)
        mean, std = dec.predict_tensor([rows], return_std=True)
        report(what="std", **spread(ms_std), pieces=len(pieces), rows_per_piece=pieces[0][1] - pieces[0][0],
               workspace_bytes=4 * Np * B * (pieces[0][1] - pieces[0][0]), mean_std=float(std[:, :ag._B].mean()), **common)

        Tp = pieces[0][1] - pieces[0][0]
        part = rows[:Tp]
        Mp = Tp * B
        wts, sq, al = dec._device_tables(rows.device)
        linv_t = dec._variance_table(rows.device)
        inv = 1.0 / (2.0 * dec.length_scale ** 2)
        ws = torch.empty(Tp * Np * B, dtype=torch.float32, device=rows.device)
        var = torch.empty((Tp, B), dtype=torch.float32, device=rows.device)
        out = torch.empty((Tp, 2, B), dtype=torch.float32, device=rows.device)
        arr = (L.RiabFFInput * 1)()
        arr[0].rates, arr[0].wt, arr[0].n_in = part.data_ptr(), wts[0].data_ptr(), n

        def abi():
            L.check(L.lib.riab_gp_predict_var(arr, 1, L.ptr(sq), L.ptr(al), 2, N, inv, L.ptr(linv_t), Tp, B, L.ptr(ws), L.ptr(var),
                                              L.ptr(out), L.current_stream()), "riab_gp_predict_var")
        ms_abi = events(abi, a.repeats)
        med_abi = statistics.median(ms_abi)
        report(what="abi", **spread(ms_abi), rows_timed=Tp, queries_timed=Mp, n_train_padded=Np, **common)

        ms_mean = events(lambda: dec.predict_tensor([part]), a.repeats)
        med_mean = statistics.median(ms_mean)
        report(what="mean", **spread(ms_mean), rows_timed=Tp, abi_over_mean=round(med_abi / med_mean, 2),
               cross_term_TFLOPs=round(2.0 * n * Np * Mp / med_mean * 1e-9, 2), **common)

        try:
            st = stage_times(abi, a.repeats)
            s1, s2 = st.get("gp_kernel", 0.0) * 1e-3, st.get("gp_var_kernel", 0.0) * 1e-3
            report(what="stages", stage1_ms=round(s1, 3), stage2_ms=round(s2, 3), sum_ms=round(s1 + s2, 3),
                   abi_ms_median=round(med_abi, 3), stage2_nominal_TFLOPs=round(Mp * float(Np) ** 2 / s2 * 1e-9, 2) if s2 else None,
                   stage2_multiplied_TFLOPs=round(Mp * float(Np) ** 2 * (1 + 128.0 / Np) / s2 * 1e-9, 2) if s2 else None,
                   stage1_over_mean=round(s1 / med_mean, 2) if s1 else None, workspace_write_GBs=round(4.0 * Np * Mp / s1 * 1e-6, 1)
                   if s1 else None, workspace_read_bytes_nominal=int(4.0 * Mp * Np * (Np / 128 + 1) / 2), rows_timed=Tp, **common)
        except Exception as e:  # the profiler is a convenience: the event-timed figures stand without it
            report(what="stages", skipped=f"torch.profiler: {type(e).__name__}: {e}", **common)

        X32 = dec.X_train_.to(torch.float32)
        L32 = dec._factor(rows.device).to(torch.float32)
        ms_t = events(lambda: torch_route(part, X32, sq[:N], L32, inv), a.repeats)
        diff = float((torch_route(part, X32, sq[:N], L32, inv)[:, :ag._B] - var[:, :ag._B]).abs().max())
        report(what="torch", **spread(ms_t), abi_over_torch=round(med_abi / statistics.median(ms_t), 3),
               max_var_difference_from_kernel=diff, rows_timed=Tp, **common)
        del L32

        q = min(256, ag._B)
        s64 = dec.std_float64(part[0, :, :q].T.to(torch.float64))
        report(what="float64", queries=q, max_var_difference=float((s64 ** 2 - var[0, :q].to(torch.float64)).abs().max()),
               var_min=float(var[:, :ag._B].min()), var_max=float(var[:, :ag._B].max()), cells=n, n_train=N)


if __name__ == "__main__":
    main()
