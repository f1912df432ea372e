"""No-GPU checks of the Bayesian decoder's backward smoother: the oracle (tests/bayes_smoother_oracle.py) against an exact
enumeration of all paths and against the dense forward-backward passes, its invariants (sum gamma = 1, mixing = 1, restarts,
NaN windows), the two new exports in the header, the bindings and the documents, their argument errors, which come before
any launch, and what `BayesianFilter.smoothed` builds and refuses."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import bayes_filter_oracle as flt
from tests import bayes_smoother_oracle as smo
from tests.test_bayes_filter_cpu import cpu_decoder
from tests.test_gpu_filter_decoder import Problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def problem(seed, shape, T, R, mixing, B=4, widths=(5,), bad_bin=None):
    """a `Problem` of the filter's tests, all columns real; `bad_bin`: that bin (and only that one) is not admissible"""
    P = Problem(seed, widths, B, B, shape, T, R, mixing=mixing)
    if bad_bin is not None:
        assert P.ok.all()
        ok = np.ones(P.J, dtype=bool)
        ok[bad_bin] = False
        w = np.where(ok, np.exp(P.logp.astype(np.float64)), 0.0)
        with np.errstate(divide="ignore"):
            P.ok, P.logp = ok, np.log(w / w.sum()).astype(np.float32)
        P.inv_norm = flt.inv_norm(ok.reshape(shape), P.g).reshape(-1).astype(np.float32)
    return P


def smooth(P, K=None, restart=None, mixing=None, dtype=np.float64):
    run = smo.smooth_float64 if dtype == np.float64 else smo.smooth_float32
    return run(P.K if K is None else K, P.L, P.S, P.tau, P.logp, P.shape, P.g, P.mixing if mixing is None else mixing, P.centres,
               restart)


def dense(P, restart=None):
    return smo.smooth_dense(P.K, P.L, P.S, P.tau, P.logp, P.shape, P.g, P.mixing, restart)


def enumerate_paths(P):
    """gamma (T, B, J) from the weight of every path through the admissible bins: prior(j_0) prod_t T[j_t, j_t-1] exp(loglik_t)"""
    lik = smo.loglik(P.K, P.L, P.S, P.tau, P.logp)
    Tm = smo.transition_matrix(P.logp, P.shape, P.g, P.mixing)
    prior = np.exp(P.logp.astype(np.float64))
    idx = np.flatnonzero(P.ok)
    T, B, J = lik.shape
    gamma = np.zeros((T, B, J))
    for b in range(B):
        shift = lik[:, b][:, P.ok].max(axis=1)
        for path in itertools.product(idx, repeat=T):
            w = prior[path[0]] * np.exp(lik[0, b, path[0]] - shift[0])
            for t in range(1, T):
                w *= Tm[path[t], path[t - 1]] * np.exp(lik[t, b, path[t]] - shift[t])
            for t in range(T):
                gamma[t, b, path[t]] += w
    return gamma / gamma.sum(axis=2, keepdims=True)


@pytest.mark.parametrize("mixing", [1e-3, 0.3])
@pytest.mark.parametrize("shape,T,bad", [((2, 2), 4, 1), ((2, 3), 3, 4)], ids=["2x2x4", "2x3x3"])
def test_the_oracle_against_every_path(shape, T, bad, mixing):
    P = problem(3, shape, T, 1, mixing, bad_bin=bad)
    assert (~P.ok).sum() == 1
    out, gamma, filtered, total = smooth(P)
    want = enumerate_paths(P)
    err = np.abs(gamma - want).max()
    print(f"{shape} x {T} windows, mixing {mixing}: gamma off the enumeration by {err:.3g}")
    assert err <= 1e-13 and (gamma[:, :, ~P.ok] == 0).all()
    assert np.abs(total - 1.0).max() <= 1e-12
    cen = P.centres.astype(np.float64)
    assert np.abs(out[:, :, :2] - want @ cen.T).max() <= 1e-13
    assert np.array_equal(out[:, :, 4], filtered[:, :, 4])
    assert np.array_equal(out[-1], filtered[-1])                                 # the last window is the filter's
    assert np.abs(np.exp(filtered[:, :, 4].sum(axis=0)) / _evidence(P) - 1.0).max() <= 1e-12


def _evidence(P):
    """p(k_1..k_T) per column, by summing every path"""
    lik = smo.loglik(P.K, P.L, P.S, P.tau, P.logp)
    Tm = smo.transition_matrix(P.logp, P.shape, P.g, P.mixing)
    a = np.exp(P.logp.astype(np.float64))[None, :] * np.exp(lik[0])
    for t in range(1, lik.shape[0]):
        a = np.exp(lik[t]) * (a @ Tm.T)
    return a.sum(axis=1)


@pytest.mark.parametrize("shape,T,R,restart_at", [((7, 9), 24, 1, None), ((8, 8), 6, 16, 3)], ids=["7x9_R1", "8x8_R16_restart"])
def test_separable_against_dense(shape, T, R, restart_at):
    P = problem(4, shape, T, R, 1e-3)
    assert not P.ok.all()
    restart = None
    if restart_at is not None:
        restart = np.zeros((T, P.B), dtype=bool)
        restart[restart_at, :2] = True
    out, gamma, filtered, total = smooth(P, restart=restart)
    want = dense(P, restart)
    err = np.abs(gamma - want).max()
    print(f"{shape}, R {R}: gamma off the dense passes by {err:.3g}; sum p beta off 1 by {np.abs(total - 1).max():.3g}")
    assert err <= 1e-12
    assert np.abs(gamma.sum(axis=2) - 1.0).max() <= 1e-12 and np.abs(total - 1.0).max() <= 1e-11
    j = gamma.argmax(axis=2)
    cen = P.centres.astype(np.float64)
    live = ~smo.cuts(filtered, restart)
    assert np.array_equal(out[:, :, 2][live], cen[0][j][live]) and np.array_equal(out[:, :, 3][live], cen[1][j][live])
    assert np.allclose(out[:, :, 5][live], np.take_along_axis(gamma, j[:, :, None], 2)[:, :, 0][live], rtol=1e-12, atol=0)
    if restart is not None:                                                     # the window before a restart is the filter's
        assert np.array_equal(out[restart_at - 1, :2], filtered[restart_at - 1, :2])
        assert not np.array_equal(out[restart_at - 1, 2:], filtered[restart_at - 1, 2:])
    moved = np.sqrt(((out[:, :, :2] - filtered[:, :, :2]) ** 2).sum(axis=2)).max()
    assert moved > 1e-3                                                         # smoothing does something


def test_mixing_one_is_the_filter():
    P = problem(5, (5, 13), 6, 2, 1.0)
    out, gamma, filtered, _ = smooth(P)
    assert np.allclose(out, filtered, rtol=1e-12, atol=1e-13)


def test_a_restart_is_two_runs():
    P = problem(6, (7, 9), 8, 1, 1e-3)
    restart = np.zeros((8, P.B), dtype=bool)
    restart[5] = True
    out = smooth(P, restart=restart)[0]
    left, right = smooth(P, K=P.K[:5])[0], smooth(P, K=P.K[5:])[0]
    assert np.array_equal(out[:5], left) and np.array_equal(out[5:], right)
    assert not np.array_equal(out[:5], smooth(P)[0][:5])


def test_a_nan_window_cuts_both_sides():
    P = problem(7, (7, 9), 8, 1, 1e-3)
    K = P.K.astype(np.float64)
    K[4, 1, 0] = np.nan
    out, gamma, filtered, _ = smooth(P, K=K)
    assert np.isnan(out[4, 1]).all() and np.isfinite(np.delete(out, 4, axis=0)[:, 1]).all()
    left, right = smooth(P, K=P.K[:4])[0], smooth(P, K=P.K[5:])[0]
    assert np.array_equal(out[:4, 1], left[:, 1]) and np.array_equal(out[5:, 1], right[:, 1])
    assert np.array_equal(out[3, 1], filtered[3, 1])
    others = [0, 2, 3]
    assert np.allclose(out[:, others], smooth(P)[0][:, others], rtol=1e-12, atol=1e-14)      # (NumPy's own sums may reorder)


def test_float32_yardstick_is_close():
    P = problem(8, (7, 9), 12, 1, 1e-3)
    o64, o32 = smooth(P)[0], smooth(P, dtype=np.float32)[0]
    assert o32.dtype == np.float32 and np.abs(o32[:, :, :2] - o64[:, :, :2]).max() < 1e-5


# ---- the surface ------------------------------------------------------------------------------------------------------------
def test_the_exports_are_declared_bound_and_documented():
    from ratinabox_amd import _build, _lib, ops
    import ratinabox_amd as riab
    header = open(os.path.join(ROOT, "include", "riab_hip.h")).read()
    assert int(re.search(r"#define RIAB_ABI_VERSION (\d+)", header).group(1)) == 11 == _lib.ABI_VERSION == _lib.lib.riab_abi_version()
    for name in ("riab_bayes_smooth", "riab_bayes_filter_keep"):
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.PROTOTYPES and hasattr(_lib.lib, name)
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "riab_bayes_smooth.hip" in _build.SOURCES
    assert hasattr(torch.ops.riab, "bayes_smooth") and hasattr(torch.ops.riab, "bayes_filter_keep")
    for Jp, S in ((32, 1), (96, 3), (416, 13), (512, 16), (544, 5), (4096, 32)):
        assert ops.bayes_smooth_workspace_floats(Jp, 132) == (5 * S + (S + 3) // 4 + 1) * 132
    assert "RIAB_BAYES_SMOOTH_WORKSPACE_FLOATS" in header
    assert "BayesianSmoother" in riab.__all__ and issubclass(riab.BayesianSmoother, riab._decoder.HistoryDecoder)
    for doc in ("DESIGN.md", "README.md"):
        assert "smoothed()" in open(os.path.join(ROOT, doc)).read(), doc


def test_argument_errors_before_launch():
    """Negative codes come from validation only: no device is needed, nothing is launched."""
    from ratinabox_amd import _lib as L
    p = C.c_void_p(256)
    g = (C.c_float * 17)(*([0.5] + [0.25] * 16))

    def smooth_call(loglik=p, ells=p, filtered=p, W=2, J=63, Jp=64, ny=7, nx=9, B=8, radius=1, taps=g, mixing=1e-3, prior=p,
                    inv_norm=p, centres=p, restart=None, last=1, beta=p, tmp=p, ws=p, out=p):
        return L.lib.riab_bayes_smooth(loglik, ells, filtered, W, J, Jp, ny, nx, B, radius, taps, mixing, prior, inv_norm, centres,
                                       restart, last, beta, tmp, ws, out, None)

    def keep_call(loglik=p, W=2, J=63, Jp=64, ny=7, nx=9, B=8, radius=1, taps=g, mixing=1e-3, prior=p, inv_norm=p, centres=p,
                  restart=None, first=1, ells=p, tmp=p, ws=p, out=p):
        return L.lib.riab_bayes_filter_keep(loglik, W, J, Jp, ny, nx, B, radius, taps, mixing, prior, inv_norm, centres, restart,
                                            first, ells, tmp, ws, out, None)
    bad = (C.c_float * 17)(*([0.5, float("nan")] + [0.0] * 15))
    for call, pointers in ((smooth_call, ("loglik", "ells", "filtered", "prior", "inv_norm", "centres", "beta", "tmp", "ws", "out")),
                           (keep_call, ("loglik", "prior", "inv_norm", "centres", "ells", "tmp", "ws", "out"))):
        assert call(W=0) == 0                                                   # nothing to do, nothing launched
        for name in pointers + ("taps",):
            assert call(**{name: None}) == L.EINVAL, name
        for kw in (dict(W=-1), dict(J=0), dict(Jp=32), dict(ny=7, nx=8), dict(ny=0, nx=0), dict(B=0), dict(radius=0),
                   dict(radius=17), dict(mixing=0.0), dict(mixing=1.5), dict(mixing=float("nan")), dict(mixing=-0.5)):
            assert call(**kw) == L.EINVAL, kw
        assert call(taps=bad) == L.EINVAL
        assert call(J=4097, Jp=4128, ny=1, nx=4097) == L.EUNSUPPORTED
        assert call(B=6) == L.EALIGN and call(J=63, Jp=63) == L.EALIGN
        for name in pointers:
            assert call(**{name: C.c_void_p(260)}) == L.EALIGN, name
        assert call(W=65536) == L.ETOOBIG and call(B=64 * 2 ** 31 + 4) == L.ETOOBIG


def test_smoothed_and_the_state_budget():
    import ratinabox_amd as riab
    dec, _ok = cpu_decoder(grid_shape=(5, 13), bin_width=0.05)
    filt = dec.with_continuity(sigma=0.03)
    sm = filt.smoothed()
    assert isinstance(sm, riab.BayesianSmoother) and sm.filter is filt and sm.decoder is dec and sm.max_state_bytes == 2 ** 31
    assert sm.window == filt.window and sm.target == "pos"
    Jp = 96
    per_column = 4 * 10 * Jp                                                    # ten windows of l, one column
    assert sm.column_blocks(10, 256) == (True, [(0, 256)])
    assert filt.smoothed(2 * per_column * 256).column_blocks(10, 256) == (True, [(0, 256)])
    assert filt.smoothed(2 * per_column * 256 - 1).column_blocks(10, 256) == (False, [(0, 256)])
    assert filt.smoothed(per_column * 256 - 1).column_blocks(10, 256) == (False, [(0, 192), (192, 256)])
    assert filt.smoothed(per_column * 128).column_blocks(10, 260) == (False, [(0, 128), (128, 256), (256, 260)])
    assert filt.smoothed(per_column * 64).column_blocks(10, 132) == (False, [(0, 64), (64, 128), (128, 132)])
    assert filt.smoothed(per_column * 4).column_blocks(10, 4) == (False, [(0, 4)])
    with pytest.raises(ValueError, match=rf"{per_column * 64} bytes.*max_state_bytes is {per_column * 64 - 1}\b"):
        filt.smoothed(per_column * 64 - 1).column_blocks(10, 132)
    with pytest.raises(ValueError, match=rf"{per_column * 4} bytes.*max_state_bytes is 100\b"):
        filt.smoothed(100).column_blocks(10, 4)
    for wrong in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="max_state_bytes"):
            filt.smoothed(wrong)
    with pytest.raises(ValueError, match="estimate"):
        sm.decode_tensor(estimate="median")
