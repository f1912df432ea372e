"""No-GPU checks of the Bayesian decoder's forward filter: the oracle's separable transition against the dense matrix of the
definition, the taps and the radius rule, what `BayesianDecoder.with_continuity` builds and refuses, the new export in the
header, the bindings and the documents, and the argument errors of `riab_bayes_filter`, which come before any launch."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import bayes_filter_oracle as flt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(1, 1), (1, 33), (7, 9), (5, 13)]


def mask(shape, seed=0):
    """about a tenth of the bins inadmissible (none on a single bin), one bin always admissible"""
    rng = np.random.RandomState(seed)
    ok = rng.rand(*shape) > 0.1 if shape != (1, 1) else np.ones(shape, dtype=bool)
    ok[shape[0] // 2, shape[1] // 2] = True
    return ok


def taps_of_radius(R, dx=0.05):
    got, g = flt.taps((R - 0.5) * dx / 3.0, dx)
    assert got == R and len(g) == 2 * R + 1
    return g


@pytest.mark.parametrize("shape", GRIDS, ids=[f"{a}x{b}" for a, b in GRIDS])
@pytest.mark.parametrize("R", [1, 2, "beyond"])
def test_separable_transition_is_the_dense_matrix(shape, R):
    R = max(shape) + 1 if R == "beyond" else R
    g = taps_of_radius(R)
    ok = mask(shape)
    assert shape == (1, 1) or not ok.all()
    T = flt.dense_transition(ok, g)
    flat = ok.reshape(-1)
    J = flat.size
    assert np.abs(T[:, flat].sum(axis=0) - 1.0).max() <= 1e-12          # every admissible source keeps its mass
    assert (T[:, ~flat] == 0).all() and (T[~flat, :] == 0).all()        # nothing leaves or reaches an inadmissible bin
    rng = np.random.RandomState(1)
    p = rng.rand(4, J) * flat
    p[0] = np.eye(J)[np.flatnonzero(flat)[0]]
    p /= p.sum(axis=1, keepdims=True)
    got = flt.propagate(p, ok, g)
    assert np.abs(got - p @ T.T).max() <= 1e-14
    assert (got[:, ~flat] == 0).all() and np.abs(got.sum(axis=1) - 1.0).max() <= 1e-12
    assert np.array_equal(flt.inv_norm(ok, g) > 0, ok)


def test_taps_and_the_radius_rule():
    from ratinabox_amd._bayes_decoder import FILTER_MAX_RADIUS, continuity_taps
    assert FILTER_MAX_RADIUS == 16
    for sigma, dx, R in ((0.004, 0.05, 1), (0.0167, 0.05, 2), (0.02, 0.05, 2), (0.049, 0.05, 3), (0.26, 0.05, 16), (0.099, 0.02, 15)):
        got, g = continuity_taps(sigma, dx)
        want, gw = flt.taps(sigma, dx)
        assert got == want == R == max(1, int(np.ceil(3 * sigma / dx))) and g.dtype == np.float64
        assert np.array_equal(g, gw) and abs(g.sum() - 1.0) <= 1e-15 and np.array_equal(g, g[::-1]) and g[R] == g.max()
        d = np.arange(-R, R + 1) * dx
        assert np.allclose(g / g[R], np.exp(-d * d / (2 * sigma * sigma)), rtol=1e-14)
    with pytest.raises(ValueError, match="sigma"):
        continuity_taps(0.0, 0.05)
    with pytest.raises(ValueError, match="sigma"):
        continuity_taps(-0.1, 0.05)
    with pytest.raises(ValueError, match=r"sigma.*0\.05"):       # R = 17: named, not truncated
        continuity_taps(0.27, 0.05)


def cpu_decoder(shape=(5, 13), dx=0.05, speed=0.08, window=2, **kw):
    """a decoder from bare tuning curves on the host, with a grid and a stand-in population for the default sigma"""
    import ratinabox_amd as riab
    rng = np.random.RandomState(2)
    ny, nx = shape
    J = ny * nx
    X, Y = np.meshgrid((np.arange(nx) + 0.5) * dx, ((np.arange(ny) + 0.5) * dx)[::-1])
    centres = np.stack((X.reshape(-1), Y.reshape(-1)))
    ok = mask(shape, 3).reshape(-1)
    f = 10.0 * rng.rand(6, J)
    pop = types.SimpleNamespace(Agent=types.SimpleNamespace(speed_mean=speed))
    dec = riab.BayesianDecoder.from_tuning([torch.from_numpy(f)], torch.from_numpy(centres), 0.05, admissible=torch.from_numpy(ok),
                                           prior_weights=torch.from_numpy(1.0 + rng.rand(J)), window=window, populations=[pop], **kw)
    return dec, ok


def test_with_continuity_builds_the_oracles_tables():
    import ratinabox_amd as riab
    dec, ok = cpu_decoder(grid_shape=(5, 13), bin_width=0.05)
    assert dec.bin_width == 0.05
    filt = dec.with_continuity(sigma=0.03, mixing=0.25)
    assert isinstance(filt, riab.BayesianFilter) and filt.radius == 2 and filt.mixing == 0.25 and filt.sigma == 0.03
    R, g = flt.taps(0.03, 0.05)
    assert np.array_equal(filt.taps, g) and filt._taps32 == [float(np.float32(v)) for v in g[R:]]
    Jp = 96
    assert tuple(filt.inv_norm.shape) == tuple(filt.prior.shape) == (Jp,) and filt.inv_norm.dtype == filt.prior.dtype == torch.float32
    want = flt.inv_norm(ok.reshape(5, 13), g).reshape(-1)
    assert np.array_equal(filt.inv_norm.numpy()[:65], want.astype(np.float32)) and (filt.inv_norm.numpy()[65:] == 0).all()
    logp = dec.log_prior.numpy().astype(np.float64)
    assert np.array_equal(filt.prior.numpy(), np.exp(logp).astype(np.float32)) and (filt.prior.numpy()[65:] == 0).all()
    assert np.array_equal(filt.prior.numpy()[:65] > 0, ok)
    bias = filt._lik_bias(2).numpy()
    assert np.array_equal(np.isfinite(bias[:65]), ok) and np.isinf(bias[65:]).all()
    assert np.array_equal(bias[:65][ok], (-0.1 * dec.S.numpy().astype(np.float64)[:65][ok]).astype(np.float32))
    # the default sigma: speed_mean x window x dt, floored at half a bin
    assert dec.with_continuity().sigma == 0.5 * 0.05 and dec.with_continuity().mixing == 1e-3            # 0.08 * 2 * 0.05 = 0.008
    fast, _ = cpu_decoder(speed=0.45, window=4, grid_shape=(5, 13), bin_width=0.05)
    assert fast.with_continuity().sigma == pytest.approx(0.45 * 4 * 0.05) and fast.with_continuity().radius == 6


def test_what_with_continuity_refuses():
    bare, _ = cpu_decoder()
    assert bare.grid_shape is None and bare.bin_width is None
    with pytest.raises(ValueError, match="grid"):
        bare.with_continuity(sigma=0.05)
    dec, _ = cpu_decoder(grid_shape=(5, 13), bin_width=0.05)
    for sigma in (0.0, -1.0):
        with pytest.raises(ValueError, match="sigma"):
            dec.with_continuity(sigma=sigma)
    with pytest.raises(ValueError, match=r"sigma.*0\.05"):
        dec.with_continuity(sigma=0.3)
    for mixing in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="mixing"):
            dec.with_continuity(sigma=0.05, mixing=mixing)
    assert dec.with_continuity(sigma=0.05, mixing=1.0).mixing == 1.0
    wrong, _ = cpu_decoder(grid_shape=(5, 12), bin_width=0.05)
    with pytest.raises(ValueError, match="grid"):
        wrong.with_continuity(sigma=0.05)


def test_the_export_is_declared_bound_and_documented():
    from ratinabox_amd import _build, _lib, ops
    header = open(os.path.join(ROOT, "include", "riab_hip.h")).read()
    assert int(re.search(r"#define RIAB_ABI_VERSION (\d+)", header).group(1)) == 11 == _lib.ABI_VERSION == _lib.lib.riab_abi_version()
    assert re.search(r"\bint riab_bayes_filter\(", header) and "riab_bayes_filter" in _lib.PROTOTYPES
    assert hasattr(_lib.lib, "riab_bayes_filter") and "riab_bayes_filter.hip" in _build.SOURCES
    assert int(re.search(r"#define RIAB_BAYES_FILTER_MAX_RADIUS (\d+)", header).group(1)) == _lib.BAYES_FILTER_MAX_RADIUS == 16
    assert hasattr(torch.ops.riab, "bayes_filter")
    for Jp, S in ((32, 1), (96, 3), (416, 13), (512, 16), (544, 5), (4096, 32)):     # the header's formula
        assert ops.bayes_filter_splits(Jp) == S and ops.bayes_filter_workspace_floats(Jp, 132) == (5 * S + 1) * 132
    assert "(Jp) <= 512 ? (Jp) / 32 : ((Jp) + 127) / 128" in header
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "with_continuity" in text or "riab_bayes_filter" in text, doc
    assert "riab_bayes_filter" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_argument_errors_before_launch():
    """Negative codes come from validation only: no device is needed, nothing is launched."""
    from ratinabox_amd import _lib as L
    p = C.c_void_p(256)
    g = (C.c_float * 17)(*([0.5] + [0.25] * 16))

    def call(loglik=p, W=2, J=63, Jp=64, ny=7, nx=9, B=8, radius=1, taps=g, mixing=1e-3, prior=p, inv_norm=p, centres=p,
             restart=None, first=1, post=p, tmp=p, ws=p, out=p):
        return L.lib.riab_bayes_filter(loglik, W, J, Jp, ny, nx, B, radius, taps, mixing, prior, inv_norm, centres, restart,
                                       first, post, tmp, ws, out, None)
    assert call(W=0) == 0                                                       # nothing to do, nothing launched
    for name in ("loglik", "prior", "inv_norm", "centres", "post", "tmp", "ws", "out", "taps"):
        assert call(**{name: None}) == L.EINVAL, name
    for kw in (dict(W=-1), dict(J=0), dict(Jp=32), dict(ny=7, nx=8), dict(ny=0, nx=0), dict(B=0), dict(radius=0), dict(radius=17),
               dict(mixing=0.0), dict(mixing=1.5), dict(mixing=float("nan")), dict(mixing=-0.5)):
        assert call(**kw) == L.EINVAL, kw
    bad = (C.c_float * 17)(*([0.5, float("nan")] + [0.0] * 15))
    assert call(taps=bad) == L.EINVAL
    assert call(J=4097, Jp=4128, ny=1, nx=4097) == L.EUNSUPPORTED
    assert call(B=6) == L.EALIGN and call(J=63, Jp=63) == L.EALIGN
    for name in ("loglik", "prior", "inv_norm", "centres", "post", "tmp", "ws", "out"):
        assert call(**{name: C.c_void_p(260)}) == L.EALIGN, name
    assert call(W=65536) == L.ETOOBIG and call(B=64 * 2 ** 31 + 4) == L.ETOOBIG
