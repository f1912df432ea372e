"""The Bayesian decoder's backward smoother on the device (csrc/riab_bayes_smooth.hip, riab_bayes_filter_keep in
csrc/riab_bayes_filter.hip, BayesianSmoother in ratinabox_amd/_bayes_decoder.py) against the float64 restatement
(tests/bayes_smoother_oracle.py).  The kernel tests write their own tables and call the three operators themselves: feedforward
for the likelihood, bayes_filter_keep for the forward scan, bayes_smooth for the backward one.  The shapes are those of
tests/test_gpu_filter_decoder.py (`CASES`, `MOST_BINS`): the smallest at which these kernels, which have the filter's structure,
can go wrong.

The tolerance is a measured one.  `smooth_float32` is the oracle's recursion in plain float32 NumPy; over `CASES` its largest
posterior-mean difference from the float64 oracle is d32, and its largest difference in log gamma over the bins with gamma > 1e-6
is Delta.  Asserted per (window, column): the device's MAP bin is admissible and the oracle's log gamma there is within Delta of
the oracle's maximum; the device's smoothed mean is within max(16 d32, 1e-6 m) of the oracle's (the factor and the floor of the
filter's own measured-tolerance test)."""
import numpy as np
import pytest
import torch

from tests import bayes_smoother_oracle as smo
from tests.guard_arena import CANARIES, GuardArena
from tests.test_gpu_filter_decoder import BIN, CASES, DEV, DT, FLOOR, IDS, MOST_BINS, PEAK, Problem, bin_of, bits, padded

pytestmark = pytest.mark.gpu


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_loglik(P, K):
    """K (T, B, n) counts (uint8, or float32 taken as counts) -> loglik (T, Jp, B) on the device"""
    x, wts, k = [], [], 0
    for w in P.widths:
        x.append(to_dev(K[:, :, k:k + w].transpose(0, 2, 1).astype(np.float32)))
        wts.append(to_dev(padded(P.L[k:k + w], P.Jp)))
        k += w
    bias = np.where(P.ok, (-np.float64(P.tau) * P.S.astype(np.float64)), -np.inf).astype(np.float32)
    return torch.ops.riab.feedforward(x, wts, to_dev(padded(bias, P.Jp)), 0, [0.0, 0.0, 0.0, 0.0])


def device_smooth(P, K=None, restart=None, batch=None, mixing=None, arena=None):
    """The forward scan with l kept, then the backward scan, in calls of `batch` windows (None: one call each) ->
    (smoothed (T, 6, B), filtered (T, 6, B)) NumPy; with `arena`, every tensor the scans write is a view inside its guard
    bands, and the views are returned: (ells, forward tmp, forward workspace, filtered, beta, tmp, workspace, out)."""
    import ratinabox_amd.ops as ops
    K = P.K if K is None else K
    T, B = K.shape[:2]
    loglik = device_loglik(P, K)
    assert tuple(loglik.shape) == (T, P.Jp, B)
    if arena is None:
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=DEV)   # noqa: E731
    else:
        new = lambda *shape: arena.view(shape, torch.float32, DEV)   # noqa: E731
    ells, ftmp, fws, filtered = new(T, P.Jp, B), new(P.Jp, B), new(ops.bayes_filter_workspace_floats(P.Jp, B)), new(T, 6, B)
    beta, tmp, ws, out = new(P.Jp, B), new(P.Jp, B), new(ops.bayes_smooth_workspace_floats(P.Jp, B)), new(T, 6, B)
    tables = ([float(v) for v in P.g32[P.R:]], P.mixing if mixing is None else mixing, to_dev(padded(P.prior, P.Jp)),
              to_dev(padded(P.inv_norm, P.Jp)), to_dev(padded(P.centres, P.Jp)))
    flags = None if restart is None else to_dev(np.asarray(restart, dtype=np.uint8))
    step = T if batch is None else batch
    starts = list(range(0, T, step))
    for o in starts:
        torch.ops.riab.bayes_filter_keep(loglik[o:o + step], P.J, P.shape[0], P.shape[1], *tables,
                                         None if flags is None else flags[o:o + step], o == 0, ells[o:o + step], ftmp, fws,
                                         filtered[o:o + step])
    for o in reversed(starts):
        torch.ops.riab.bayes_smooth(loglik[o:o + step], ells[o:o + step], filtered[o:o + step], P.J, P.shape[0], P.shape[1], *tables,
                                    None if flags is None else flags[o:o + step], o == starts[-1], beta, tmp, ws, out[o:o + step])
    torch.cuda.synchronize()
    if arena is not None:
        return ells, ftmp, fws, filtered, beta, tmp, ws, out
    return out.cpu().numpy(), filtered.cpu().numpy()


def oracle(P, K=None, restart=None, dtype=np.float64, mixing=None):
    """(outputs (T, n_real, 6), gamma (T, n_real, J), the filter's outputs) of the real columns"""
    K = P.K if K is None else K
    run = smo.smooth_float64 if dtype == np.float64 else smo.smooth_float32
    return run(K[:, :P.n_real], P.L, P.S, P.tau, P.logp, P.shape, P.g, P.mixing if mixing is None else mixing, P.centres,
               None if restart is None else restart[:, :P.n_real])[:3]


def yardstick(P):
    """(largest mean difference (m), largest log gamma difference over the bins with gamma > 1e-6) of smooth_float32 from
    smooth_float64 on this problem"""
    o64, g64, _ = oracle(P)
    o32, g32, _ = oracle(P, dtype=np.float32)
    big = g64 > 1e-6
    with np.errstate(divide="ignore"):
        dlog = np.abs(np.log(g32.astype(np.float64)[big]) - np.log(g64[big])).max()
    return float(np.abs(o32[:, :, :2].astype(np.float64) - o64[:, :, :2]).max()), float(dlog)


@pytest.fixture(scope="module")
def runs():
    """every case once: (problem, smoothed and filtered from the device, the float64 oracle's outputs and gamma); and the
    float32 yardstick (d32, Delta) over the cases"""
    out, d32, delta = {}, 0.0, 0.0
    for case, name in zip(CASES, IDS):
        P = Problem(5, *case)
        got, filtered = device_smooth(P)
        want, gamma, _ = oracle(P)
        out[name] = (P, got, filtered, want, gamma)
        d, dl = yardstick(P)
        print(f"{name}: float32 NumPy is off the float64 oracle by {d:.3g} m in the mean, {dl:.3g} in log gamma")
        d32, delta = max(d32, d), max(delta, dl)
    return out, d32, delta


def check_against_oracle(P, got, want, gamma, d32, delta, what, bound=True):
    """-> (the largest mean difference, the largest shortfall of the oracle's log gamma at the device's MAP bin)"""
    g = got[:, :, :P.n_real].transpose(0, 2, 1).astype(np.float64)                 # (T, n_real, 6)
    assert np.isfinite(g).all() and np.isfinite(want).all()
    j = bin_of(P.centres, g[:, :, 2:4].reshape(-1, 2).astype(np.float32)).reshape(g.shape[:2])
    assert P.ok[j].all()
    with np.errstate(divide="ignore"):
        lg = np.log(gamma)
    short = float((lg.max(axis=2) - np.take_along_axis(lg, j[:, :, None], axis=2)[:, :, 0]).max())
    mean = float(np.abs(g[:, :, :2] - want[:, :, :2]).max())
    prob = float(np.abs(g[:, :, 5] - want[:, :, 5]).max())
    print(f"{what}: mean off by {mean:.3g} m (allowed {max(16 * d32, 1e-6):.3g}); MAP short of the maximum by {short:.3g} in log gamma "
          f"(allowed {delta:.3g}); MAP probability off by {prob:.3g}")
    if bound:
        assert short <= delta
        assert mean <= max(16.0 * d32, 1e-6)
    return mean, short


# ---- 1. against the float64 oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_against_the_float64_oracle(runs, name):
    """Measured on an MI355X over `CASES`: d32 = 4.24e-7 m (grid (32, 64)) and Delta = 7.94e-6 (grid (7, 9), T' = 24).  The
    kernel's largest mean difference from the float64 oracle is 2.75e-7 m (populations (5, 33), B = 132, grid (3, 43), T' = 1:
    a cut window, the filter's own figure) and 2.07e-7 m among the smoothed windows (grid (20, 20), B = 132): a factor of 0.65
    where 16 is allowed.  The device's MAP bin is the oracle's in every (window, column): shortfall 0 (also in DESIGN.md
    section 5)."""
    cases, d32, delta = runs
    P, got, filtered, want, gamma = cases[name]
    assert got.shape == (P.T, 6, P.B) and got.dtype == np.float32
    check_against_oracle(P, got, want, gamma, d32, delta, name)
    assert np.array_equal(bits(got[:, 4]), bits(filtered[:, 4]))                   # row 4 is the filter's, unchanged
    assert np.array_equal(bits(got[-1]), bits(filtered[-1]))                       # the last window is the filter's


def test_most_bins_runs():
    """The (64, 64) grid, 32 ranges: its figures are printed, no bound is asserted."""
    P = Problem(5, *MOST_BINS)
    got, filtered = device_smooth(P)
    want, gamma, _ = oracle(P)
    d, dl = yardstick(P)
    check_against_oracle(P, got, want, gamma, d, dl, "most bins", bound=False)
    assert np.array_equal(bits(got[-1]), bits(filtered[-1])) and not np.array_equal(bits(got[0, :2]), bits(filtered[0, :2]))


# ---- 2. smoothing happens ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, c in zip(IDS, CASES) if c[4] > 1])
def test_smoothing_moves_the_mean(runs, name):
    P, got, filtered, _want, _gamma = runs[0][name]
    moved = np.sqrt(((got[:, :2, :P.n_real] - filtered[:, :2, :P.n_real]).astype(np.float64) ** 2).sum(axis=1))
    print(f"{name}: the smoothed mean is up to {moved.max():.3g} m from the filtered one")
    assert moved.max() > 1e-3


# ---- 3. bit-level reproducibility -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [2, 4, 8])
def test_a_column_alone_has_the_bits_it_has_among_132(case):
    P = Problem(8, *CASES[case])
    assert P.B == 132
    full = device_smooth(P)[0]
    for b in (0, 67, 129):
        one = Problem(8, *CASES[case])
        one.B, one.n_real = 4, 1
        K = np.zeros((P.T, 4, P.n), dtype=np.uint8)
        K[:, 0] = P.K[:, b]
        K[:, 1:] = 255
        assert np.array_equal(bits(device_smooth(one, K=K)[0][:, :, 0]), bits(full[:, :, b]))


@pytest.mark.parametrize("case", [2, 5, 9, -1])
def test_calls_of_one_and_of_five_windows_give_the_same_bits(case):
    P = Problem(9, *(CASES[case] if case >= 0 else MOST_BINS))
    whole, filtered = device_smooth(P)
    for batch in (1, 5):
        got, f = device_smooth(P, batch=batch)
        assert np.array_equal(bits(got[:, :, :P.n_real]), bits(whole[:, :, :P.n_real]))
        assert np.array_equal(bits(f[:, :, :P.n_real]), bits(filtered[:, :, :P.n_real]))


@pytest.mark.parametrize("case", [2, 5, 9])
def test_restarts_are_segments_run_apart_and_cut_windows_are_the_filters(runs, case):
    P = Problem(9, *CASES[case])
    T, n_real = P.T, P.n_real
    whole, _ = device_smooth(P)
    # column 0 restarts at window 1, the last real column at window T - 1
    restart = np.zeros((T, P.B), dtype=bool)
    restart[1, 0] = restart[T - 1, n_real - 1] = True
    got, filtered = device_smooth(P, restart=restart)
    for t0, b in ((1, 0), (T - 1, n_real - 1)):
        left, right = device_smooth(P, K=P.K[:t0])[0], device_smooth(P, K=P.K[t0:])[0]
        assert np.array_equal(bits(got[:t0, :, b]), bits(left[:, :, b])) and np.array_equal(bits(got[t0:, :, b]), bits(right[:, :, b]))
        assert np.array_equal(bits(got[t0 - 1, :, b]), bits(filtered[t0 - 1, :, b]))          # cut: the filter's six rows
        assert t0 < 2 or not np.array_equal(bits(got[:t0, :, b]), bits(whole[:t0, :, b]))
    assert np.array_equal(bits(got[T - 1]), bits(filtered[T - 1]))
    others = [b for b in range(n_real) if b not in (0, n_real - 1)]
    assert np.array_equal(bits(got[:, :, others]), bits(whole[:, :, others]))
    assert not np.array_equal(bits(got[0, :2, others]), bits(filtered[0, :2, others]))         # ... and only the cut ones
    want, gamma, _ = oracle(P, restart=restart)
    check_against_oracle(P, got, want, gamma, runs[1], runs[2], f"restarts, case {case}")


def class_route(P, max_state_bytes=2 ** 31, max_windows=None):
    """a BayesianSmoother over the problem's tables -> smooth_inputs_tensor of its counts, NumPy (T, 6, B)"""
    import ratinabox_amd as riab
    tables, k = [], 0
    for w in P.widths:
        tables.append(to_dev(padded(P.L[k:k + w], P.Jp, 0.0)))
        k += w
    dec = riab.BayesianDecoder(tables, to_dev(padded(P.S, P.Jp, 0.0)), to_dev(padded(P.logp, P.Jp, -np.inf)),
                               to_dev(padded(P.centres, P.Jp, 0.0)), P.J, DT, grid_shape=P.shape, bin_width=BIN)
    filt = dec.with_continuity(sigma=(P.R - 0.5) * BIN / 3.0, mixing=P.mixing)
    assert filt.radius == P.R
    filt._max_windows_per_call = max_windows
    sm = filt.smoothed(max_state_bytes)
    x, k = [], 0
    for w in P.widths:
        x.append(to_dev(P.K[:, :, k:k + w].transpose(0, 2, 1)))
        k += w
    return sm, sm.smooth_inputs_tensor(x, 1).cpu().numpy()


@pytest.mark.parametrize("case", [2, 4])
def test_column_blocks_have_the_bits_of_one_block(runs, case):
    P = Problem(13, *CASES[case])
    assert P.B == 132
    per_column = 4 * P.T * P.Jp
    sm, one = class_route(P)
    assert sm.column_blocks(P.T, P.B) == (True, [(0, 132)])
    want, gamma, _ = oracle(P)
    check_against_oracle(P, one, want, gamma, runs[1], runs[2], f"the class, case {case}")
    for budget, blocks in ((per_column * 132, 1), (per_column * 128, 2), (per_column * 64, 3)):
        sm, got = class_route(P, budget, max_windows=7)
        keep, cols = sm.column_blocks(P.T, P.B)
        assert not keep and len(cols) == blocks
        assert np.array_equal(bits(got[:, :, :P.n_real]), bits(one[:, :, :P.n_real])), blocks
    with pytest.raises(ValueError, match="max_state_bytes"):
        class_route(P, per_column * 64 - 1)


@pytest.mark.parametrize("case", [1, 4, 9])
def test_filter_keep_has_the_bits_of_the_filter(case):
    import ratinabox_amd.ops as ops
    P = Problem(14, *CASES[case])
    T, B = P.T, P.B
    loglik = device_loglik(P, P.K)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=DEV)   # noqa: E731
    tables = ([float(v) for v in P.g32[P.R:]], P.mixing, to_dev(padded(P.prior, P.Jp)), to_dev(padded(P.inv_norm, P.Jp)),
              to_dev(padded(P.centres, P.Jp)))
    n_ws = ops.bayes_filter_workspace_floats(P.Jp, B)
    post, tmp, ws, out = new(P.Jp, B), new(P.Jp, B), new(n_ws), new(T, 6, B)
    torch.ops.riab.bayes_filter(loglik, P.J, P.shape[0], P.shape[1], *tables, None, True, post, tmp, ws, out)
    ells, tmp2, ws2, out2 = new(T, P.Jp, B), new(P.Jp, B), new(n_ws), new(T, 6, B)
    torch.ops.riab.bayes_filter_keep(loglik, P.J, P.shape[0], P.shape[1], *tables, None, True, ells, tmp2, ws2, out2)
    torch.cuda.synchronize()
    same = lambda a, b: np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))   # noqa: E731
    assert same(out2, out) and same(ells[T - 1], post) and same(tmp2, tmp) and same(ws2[:n_ws], ws[:n_ws])
    want = P.oracle()[1]                                                           # the oracle's l of every window
    got = ells.cpu().numpy()[:, :P.J, :P.n_real].transpose(0, 2, 1)
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.abs(got[np.isfinite(want)] - want[np.isfinite(want)]).max() < 1e-3
    assert np.isneginf(ells.cpu().numpy()[:, P.J:]).all()


# ---- 4. mixing = 1: nothing is carried, either way --------------------------------------------------------------------------
@pytest.mark.parametrize("case", [1, 2, 4, 7])
def test_mixing_one_is_the_filter(case):
    P = Problem(6, *CASES[case])
    got, filtered = device_smooth(P, mixing=1.0)
    g, f = got[:, :, :P.n_real], filtered[:, :, :P.n_real]
    assert np.isfinite(f).all()
    assert np.allclose(g[:, :4], f[:, :4], rtol=0, atol=1e-5 * P.diag) and np.allclose(g[:, 5], f[:, 5], rtol=1e-5, atol=0)
    assert np.array_equal(bits(g[:, 4]), bits(f[:, 4]))


# ---- 5. poison stays in its column and its window ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", [4, 5, 8])
def test_poison_stays_in_its_column_and_window(case):
    widths, B, n_real, shape, T, R = CASES[case]
    P = Problem(10, widths, B, n_real, shape, max(T, 5), R)
    clean = P.K.astype(np.float32)
    clean[:, n_real:] = 0
    base, _ = device_smooth(P, K=clean)
    assert np.isfinite(base[:, :, :n_real]).all()
    b = n_real // 2
    keep = np.arange(n_real) != b
    left, right = device_smooth(P, K=clean[:2])[0], device_smooth(P, K=clean[3:])[0]
    for poison in (np.float32(np.nan), np.float32(3.0e38), np.float32(-np.inf)):
        Kp = clean.copy()
        Kp[:, n_real:] = poison                          # every padding lane, every window
        Kp[2, b, :] = poison                             # and the counts of one real column at window 2
        got, filtered = device_smooth(P, K=Kp)
        assert np.array_equal(bits(got[:, :, :n_real][:, :, keep]), bits(base[:, :, :n_real][:, :, keep])), poison
        assert np.isnan(got[2, :, b]).all(), poison
        # either side of it: finite, and the smoothing of the windows before it, and of those after it, alone
        assert np.array_equal(bits(got[:2, :, b]), bits(left[:, :, b])) and np.array_equal(bits(got[3:, :, b]), bits(right[:, :, b]))
        assert np.isfinite(got[:2, :, b]).all() and np.isfinite(got[3:, :, b]).all()
        assert np.array_equal(bits(got[1, :, b]), bits(filtered[1, :, b]))           # cut: the filter's six rows


# ---- 6. guard bands ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 2, 4, 6, 9, -1])
def test_guard_bands_around_the_state_and_the_outputs(case):
    P = Problem(12, *(CASES[case] if case >= 0 else MOST_BINS))
    seen = None
    for canary in CANARIES:
        arena = GuardArena(canary)
        views = device_smooth(P, arena=arena, batch=2)
        now = [arena.check(v, other=None if seen is None else seen[i]) for i, v in enumerate(views)]
        seen = now
    ref = device_smooth(P)[0]
    assert np.array_equal(bits(seen[7][:, :, :P.n_real]), bits(ref[:, :, :P.n_real]))


# ---- 7. through the classes -------------------------------------------------------------------------------------------------
def test_through_the_classes():
    """64 agents in the unit room (dx 0.05: 400 bins), 24 PlaceCells of 10 Hz with spikes, 200 steps of 50 ms in windows of 5"""
    import ratinabox_amd as riab
    np.random.seed(7)
    env = riab.Environment({"dx": BIN})
    ag = riab.Agent(env, {"n_agents": 64, "dt": DT, "seed": 23})
    pcs = riab.PlaceCells(ag, {"n": 24, "widths": 0.15, "max_fr": PEAK, "save_spikes": True})
    ag.simulate(200)
    dec = riab.fit_bayesian_decoder([pcs], tuning="groundtruth", window=5, rate_floor=FLOOR)
    filt = dec.with_continuity()
    sm = filt.smoothed()
    assert isinstance(sm, riab.BayesianSmoother)
    out, filtered = sm.decode_all_tensor(), filt.decode_all_tensor()
    assert tuple(out.shape) == (40, 6, 64) and out.dtype == torch.float32 and out.device.type == "cuda"
    assert torch.equal(out[:, 4], filtered[:, 4]) and torch.equal(out[-1], filtered[-1]) and not torch.equal(out[:-1, :2], filtered[:-1, :2])
    # the operator route over the same counts
    _agent, window, n, flags, pieces = filt._runs(None, None, None, "spikes", None)
    assert (window, n, flags, len(pieces)) == (5, 40, None, 1)
    x = [t.to(torch.float32) for t in pieces[0][0]]
    loglik = torch.ops.riab.feedforward(x, dec.log_rates, filt._lik_bias(5), 0, [0.0, 0.0, 0.0, 0.0])
    Jp = 416
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=DEV)   # noqa: E731
    from ratinabox_amd import ops
    tables = (filt._taps32, filt.mixing, filt.prior, filt.inv_norm, dec.centres)
    ells, tmp, fws, f2 = new(40, Jp, 64), new(Jp, 64), new(ops.bayes_filter_workspace_floats(Jp, 64)), new(40, 6, 64)
    torch.ops.riab.bayes_filter_keep(loglik, 400, 20, 20, *tables, None, True, ells, tmp, fws, f2)
    beta, ws, o2 = new(Jp, 64), new(ops.bayes_smooth_workspace_floats(Jp, 64)), new(40, 6, 64)
    torch.ops.riab.bayes_smooth(loglik, ells, f2, 400, 20, 20, *tables, None, True, beta, tmp, ws, o2)
    assert torch.equal(f2, filtered) and torch.equal(o2, out)
    # batches of windows, a budget that drops the kept likelihood, restart flags
    filt._max_windows_per_call = 7
    assert torch.equal(sm.decode_all_tensor(), out)
    assert torch.equal(filt.smoothed(4 * 40 * Jp * 64).decode_all_tensor(), out)
    filt._max_windows_per_call = None
    assert torch.equal(sm.decode_tensor(), out[:, 0:2]) and torch.equal(sm.decode_tensor(estimate="map"), out[:, 2:4])
    restart = np.zeros((40, 64), dtype=bool)
    restart[10, 3] = True
    got = sm.decode_all_tensor(restart=restart)
    t10 = np.asarray(ag.history["t"])[50]
    assert torch.equal(got[10:, :, 3], sm.decode_all_tensor(t_start=t10)[:, :, 3]) and torch.equal(got[:, :, :3], out[:, :, :3])
    assert torch.equal(got[9, :, 3], filt.decode_all_tensor(restart=restart)[9, :, 3])
    # decode() / error(), and what smoothing buys on this run (printed, not asserted)
    dd = sm.decode()
    pos = ag.get_history_tensor().cpu().numpy()[2::5, :2, :64].transpose(0, 2, 1).astype(np.float64)
    e_sm, e_filt, e_dec = float(sm.error().mean()), float(filt.error().mean()), float(dec.error().mean())
    assert dd.shape == (40, 64, 2) and tuple(sm.error().shape) == (64,)
    assert np.isclose(np.sqrt(((dd - pos) ** 2).sum(axis=2)).mean(), e_sm, rtol=1e-9)
    print(f"mean error over 40 windows of 250 ms, 64 agents: memoryless {e_dec:.4f} m, filtered {e_filt:.4f} m, smoothed {e_sm:.4f} m")
    # the oracle on the host over the device's recorded spikes
    K = np.ascontiguousarray(pieces[0][0][0].cpu().numpy().transpose(0, 2, 1))      # (40, 64, 24) counts
    J = 400
    g = np.asarray(filt._taps32[::-1][:-1] + filt._taps32, dtype=np.float64)
    want = smo.smooth_float64(K, dec.log_rates[0].cpu().numpy()[:, :J], dec.S.cpu().numpy()[:J], 5 * DT, dec.log_prior.cpu().numpy()[:J],
                              (20, 20), g, filt.mixing, dec.centres.cpu().numpy()[:, :J])[0]
    y32 = smo.smooth_float32(K, dec.log_rates[0].cpu().numpy()[:, :J], dec.S.cpu().numpy()[:J], 5 * DT, dec.log_prior.cpu().numpy()[:J],
                             (20, 20), g, filt.mixing, dec.centres.cpu().numpy()[:, :J])[0]
    off = np.abs(out.cpu().numpy()[:, :2].transpose(0, 2, 1) - want[:, :, :2]).max()
    d32 = np.abs(y32[:, :, :2].astype(np.float64) - want[:, :, :2]).max()
    print(f"the smoothed mean is off the float64 oracle by {off:.3g} m (float32 NumPy: {d32:.3g} m)")
    assert off <= max(16.0 * d32, 1e-6)
