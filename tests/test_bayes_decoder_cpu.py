"""No-GPU checks of the Bayesian decoder: the properties of the tests' float64 oracle (tests/bayes_oracle.py), the ABI of
riab_history_window_counts and riab_bayes_decode with every refusal produced by validation alone, the class-level refusals on
device="cpu" objects, and the window bookkeeping of the Python walk over history chunks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import bayes_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "riab_hip.h")


@pytest.fixture(scope="module")
def L():
    from ratinabox_amd import _lib
    return _lib


def problem(seed, n=7, J=40, S=5):
    rng = np.random.RandomState(seed)
    centres = np.stack((rng.rand(J) * 1.5, rng.rand(J)))
    f = 10.0 * rng.rand(n, J) ** 3
    k = rng.poisson(0.25 * f[:, rng.randint(0, J, size=S)].T)
    return f, k, centres


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def test_oracle_zero_counts_give_the_softmax_of_the_bias():
    f, _k, centres = problem(0)
    Lt, S, logp = orc.tables(f, prior_weights=np.arange(1, 41))
    b = orc.bias(logp, S, 0.25)
    out = orc.decode(np.zeros((1, 7)), Lt, b, centres)[0]
    p = np.exp(b - b.max())
    p /= p.sum()
    assert np.allclose(out[:2], centres @ p, rtol=1e-14) and np.isclose(out[5], p.max(), rtol=1e-14)
    assert np.isclose(out[4], np.log(np.exp(b).sum()), rtol=1e-13) and np.array_equal(out[2:4], centres[:, np.argmax(b)])
    assert np.isclose(np.exp(logp).sum(), 1.0, rtol=1e-14)                  # (the prior is normalised)


def test_oracle_ties_go_to_the_lower_index():
    f, k, centres = problem(1)
    f[:, 30] = f[:, 11]                                                       # duplicated tuning columns: equal l
    f[:, 35] = f[:, 11]
    Lt, S, logp = orc.tables(f)
    ell = orc.log_posterior(k, Lt, orc.bias(logp, S, 0.25))
    assert np.array_equal(ell[:, 11], ell[:, 30]) and np.array_equal(ell[:, 11], ell[:, 35])
    ell[:, [11, 30, 35]] += 1e3                                               # ... and the three are the maxima
    out = orc.outputs(ell, centres)
    assert (orc.map_bin(ell) == 11).all() and np.array_equal(out[:, 2:4], np.tile(centres[:, 11], (len(k), 1)))


def test_oracle_inadmissible_bins():
    f, k, centres = problem(2, J=96)
    ok = np.ones(96, dtype=bool)
    ok[:32] = False                                                           # the first block of bins
    Lt, S, logp = orc.tables(f, admissible=ok)
    assert np.isinf(logp[:32]).all() and np.isclose(logp[32], -np.log(64))
    full = orc.decode(k, Lt, orc.bias(logp, S, 0.25), centres)
    Lr, Sr, logpr = orc.tables(f[:, 32:])
    assert np.allclose(full, orc.decode(k, Lr, orc.bias(logpr, Sr, 0.25), centres[:, 32:]), rtol=1e-13, atol=0)
    none = orc.decode(k, Lt, np.full(96, -np.inf), centres)
    assert none.shape == (len(k), 6) and np.isnan(none).all()
    assert (orc.delta(k, Lt, np.full(96, -np.inf)) == 0).all() and np.isfinite(orc.delta(k, Lt, orc.bias(logp, S, 0.25))).all()


def test_oracle_float32_evaluation_and_counts():
    f, k, centres = problem(3, n=17, J=400, S=24)
    Lt, S, logp = orc.tables(f)
    b = orc.bias(logp, S, 0.25)
    d = np.abs(orc.decode_float32(k, Lt, b, centres).astype(np.float64) - orc.decode(k, Lt, b, centres))
    assert d[:, :2].max() < 1e-5 and d[:, :2].max() > 0                       # a float32 path: close, not equal
    rng = np.random.RandomState(4)
    sp = (rng.rand(11, 3, 4) < 0.3).astype(np.uint8)
    sp[:, :, 3] = 255
    c = orc.window_counts(sp, 3)
    assert c.shape == (3, 3, 4) and c.dtype == np.uint8 and np.array_equal(c[1, :, :3], sp[3:6, :, :3].sum(axis=0))
    assert (c[:, :, 3] == (3 * 255) % 256).all() and orc.window_counts(sp, 3, modulo=False)[0, 0, 3] == 765
    assert list(orc.window_of_rows(4, 6, 3, 3)) == [1, 1, 2, 2, 2, -1]


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_prototyped(L):
    raw = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, n_args in (("riab_history_window_counts", 9), ("riab_bayes_decode", 13)):
        m = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in riab_hip.h"
        assert len(m.group(1).split(",")) == n_args == len(L.PROTOTYPES[name][1]) and hasattr(L.lib, name)
    assert int(re.search(r"#define RIAB_ABI_VERSION (\d+)", raw).group(1)) == 11 == L.ABI_VERSION == L.lib.riab_abi_version()
    for name, val in (("RIAB_BAYES_MAX_WINDOW", L.BAYES_MAX_WINDOW), ("RIAB_BAYES_OUT_ROWS", L.BAYES_OUT_ROWS),
                      ("RIAB_RATEMAP_MAX_BINS", L.RATEMAP_MAX_BINS)):
        assert int(re.search(rf"#define {name} (\d+)", raw).group(1)) == val
    assert L.BAYES_MAX_WINDOW == 255 and L.BAYES_OUT_ROWS == 6 and L.RATEMAP_MAX_BINS == 4096
    assert L.lib.riab_abi_sizeof(5) == C.sizeof(L.RiabFFInput)          # (the struct the entry point reuses is unchanged)
    from ratinabox_amd import _build
    assert "riab_bayes.hip" in _build.SOURCES
    import ratinabox_amd as riab
    assert riab.BayesianDecoder is not None and callable(riab.fit_bayesian_decoder) and hasattr(riab.Neurons, "fit_bayesian_decoder")
    assert "fit_bayesian_decoder" in riab.__all__ and "BayesianDecoder" in riab.__all__


def test_window_counts_argument_errors_before_launch(L):
    p, q = 4096, 4096 + 2

    def call(rows=p, T=1, n=3, B=8, row0=0, window=5, n_windows=4, counts=p):
        return L.lib.riab_history_window_counts(rows, T, n, B, row0, window, n_windows, counts, None)
    assert call(T=0) == 0 and call(n_windows=0) == 0                       # nothing to do, nothing launched
    assert call(rows=None) == L.EINVAL and call(counts=None) == L.EINVAL
    assert call(window=0) == L.EINVAL and call(window=-1) == L.EINVAL and call(window=256) == L.EINVAL
    assert call(window=255, T=0) == 0 and call(window=1, T=0) == 0
    assert call(T=-1) == L.EINVAL and call(n=0) == L.EINVAL and call(B=0) == L.EINVAL
    assert call(row0=-1) == L.EINVAL and call(n_windows=-1) == L.EINVAL
    assert call(B=6) == L.EALIGN == -2 and call(rows=q) == L.EALIGN and call(counts=q) == L.EALIGN
    assert call(T=1 << 40) == L.ETOOBIG and call(T=1 << 20, n=1 << 10, B=1 << 12) == L.ETOOBIG
    assert call(row0=20, T=7) == 0                                          # every row lies past the last window: no launch


def test_bayes_decode_argument_errors_before_launch(L):
    p, q = 4096, 4096 + 4

    def call(rows=p, wt=p, n_in=3, n_inputs=1, counts=1, scale=0.25, bias=p, centres=p, J=40, Jp=64, T=0, B=8, out=p,
             block_tiles=0, null_inputs=False):
        arr = (L.RiabFFInput * 9)()
        for a in arr:
            a.rates, a.wt, a.n_in = rows, wt, n_in
        return L.lib.riab_bayes_decode(None if null_inputs else arr, n_inputs, counts, scale, bias, centres, J, Jp, T, B, out,
                                       block_tiles, None)
    assert call() == 0                                                            # T = 0: checked, nothing launched
    for null in ("rows", "wt", "bias", "centres", "out"):
        assert call(**{null: None}) == L.EINVAL, null
    assert call(null_inputs=True) == L.EINVAL
    assert call(n_inputs=0) == L.EINVAL and call(n_inputs=9) == L.EINVAL and call(n_inputs=8) == 0
    assert call(n_in=0) == L.EINVAL and call(n_in=-3) == L.EINVAL
    assert call(J=0) == L.EINVAL and call(J=-1) == L.EINVAL and call(J=65) == L.EINVAL and call(J=64) == 0 and call(J=1) == 0
    assert call(T=-1) == L.EINVAL and call(B=0) == L.EINVAL
    for bt in (1, 2, 4):
        assert call(block_tiles=bt) == 0
    assert call(block_tiles=3) == L.EINVAL and call(block_tiles=-1) == L.EINVAL and call(block_tiles=8) == L.EINVAL
    for bad in (float("nan"), float("inf")):
        assert call(scale=bad, counts=0) == L.EINVAL and call(scale=bad, counts=1) == 0    # (counts are not scaled)
    assert call(J=L.RATEMAP_MAX_BINS, Jp=4096) == 0 and call(J=L.RATEMAP_MAX_BINS + 1, Jp=4128) == L.EUNSUPPORTED == -4
    assert call(B=6) == L.EALIGN == -2 and call(Jp=48) == L.EALIGN and call(Jp=40) == L.EALIGN
    for mis in ("wt", "bias", "centres", "out"):
        assert call(**{mis: q}) == L.EALIGN, mis
    assert call(rows=q, counts=1) == 0 and call(rows=q, counts=0) == L.EALIGN      # counts: 4-byte rows; rates: 16-byte
    assert call(rows=p + 2, counts=1) == L.EALIGN
    assert call(T=1 << 40) == L.ETOOBIG == -3 and call(T=1 << 31, B=8) == L.ETOOBIG
    assert call(T=1 << 62, B=512) == L.ETOOBIG and call(T=1 << 61, B=1024) == L.ETOOBIG    # (T * tiles wraps in 64 bits)


# ---- the classes, on device="cpu" objects -----------------------------------------------------------------------------------
def test_class_level_refusals_on_cpu_objects():
    """Every refusal is raised before any native call: the objects live on device="cpu", where no kernel can run."""
    import torch
    import ratinabox_amd as riab
    from ratinabox_amd import _bayes_decoder as B
    np.random.seed(0)
    env = riab.Environment({})
    ag = riab.Agent(env, {"n_agents": 8, "device": "cpu"})
    other = riab.Agent(env, {"n_agents": 8, "device": "cpu"})
    pcs = riab.PlaceCells(ag, {"n": 4})
    quiet = riab.PlaceCells(ag, {"n": 3, "save_spikes": False})
    foreign = riab.PlaceCells(other, {"n": 4})
    for kw, frag in ((dict(tuning="sklearn"), "tuning"), (dict(prior="flat"), "prior"), (dict(rate_floor=0.0), "rate_floor"),
                     (dict(window=0), "window"), (dict(window=256), "window"), (dict(window=2.5), "window"),
                     (dict(prior="occupancy", tuning="groundtruth"), "occupancy")):
        with pytest.raises(ValueError, match=frag):
            riab.fit_bayesian_decoder([pcs], **kw)
    with pytest.raises(ValueError, match="one Agent"):
        riab.fit_bayesian_decoder([pcs, foreign])
    with pytest.raises(ValueError, match="1..8 populations"):
        riab.fit_bayesian_decoder([pcs] * 9)
    with pytest.raises(ValueError, match=r"grid of \d+ bins"):
        pcs.fit_bayesian_decoder(bin_size=0.0125)                               # > 80 x 80 bins (checked before the rows)
    with pytest.raises(ValueError, match="no recorded rates"):
        pcs.fit_bayesian_decoder()
    ag._hist.reserve(6)
    ag._times = [0.1 * (i + 1) for i in range(6)]
    pcs._hist_fr.reserve(6)
    quiet._hist_fr.reserve(6)
    with pytest.raises(ValueError, match="no recorded spikes"):
        pcs.fit_bayesian_decoder(spikes=True)
    with pytest.raises(ValueError, match="10000 bins"):
        pcs.fit_bayesian_decoder(tuning="groundtruth")                          # (the default Environment.dx = 0.01)
    # a decoder from bare tuning curves (host tensors): the tables, and the refusals of the decode
    f, _k, centres = problem(5, n=7, J=40)
    f[:4, 0] = 0.0
    mk = lambda pops: B.BayesianDecoder.from_tuning([torch.from_numpy(f[:4]), torch.from_numpy(f[4:])], torch.from_numpy(centres),
                                                    0.05, window=5, populations=pops)
    dec = mk(None)
    Lt, S, logp = orc.tables(f)
    assert dec.n_bins == 40 and dec.widths == [4, 3] and dec.window == 5 and tuple(dec.centres.shape) == (2, 64)
    assert np.array_equal(torch.cat(dec.log_rates)[:, :40].numpy(), Lt.astype(np.float32)) and dec.log_rates[0][0, 0] == np.float32(np.log(1e-2))
    assert np.array_equal(dec.S[:40].numpy(), S.astype(np.float32)) and np.array_equal(dec.log_prior[:40].numpy(), logp.astype(np.float32))
    assert torch.isinf(dec.log_prior[40:]).all() and not dec.S[40:].any() and not dec.centres[:, 40:].any()
    want_bias = (dec.log_prior.numpy().astype(np.float64) - 0.25 * dec.S.numpy().astype(np.float64)).astype(np.float32)
    assert np.array_equal(dec.bias().numpy(), want_bias) and np.array_equal(dec.bias(5).numpy(), want_bias)
    with pytest.raises(ValueError, match="bare tuning curves"):
        dec.decode_all_tensor()
    with pytest.raises(ValueError, match="1..4096 position bins"):
        B.BayesianDecoder.from_tuning([torch.zeros((2, 4097), dtype=torch.float64)], torch.zeros((2, 4097), dtype=torch.float64), 0.05)
    dec = mk([pcs, quiet])
    with pytest.raises(ValueError, match="window must be 1"):
        dec.decode_all_tensor(inputs="rates")                                   # (the fitted window is 5)
    with pytest.raises(ValueError, match="window must be 1"):
        dec.decode_tensor(window=2, inputs="rates")
    with pytest.raises(ValueError, match="inputs must be"):
        dec.decode_all_tensor(inputs="counts")
    with pytest.raises(ValueError, match="estimate"):
        dec.decode_tensor(estimate="median")
    with pytest.raises(ValueError, match="no recorded spikes"):
        dec.decode_all_tensor()
    pcs._hist_sp.reserve(6)
    with pytest.raises(ValueError, match="no recorded spikes"):
        dec.decode_all_tensor()                                                 # (the second population records none)
    # the centre-row targets: windows of 5 rows over 6 recorded rows -> one window, its centre row 2
    ag._hist.chunks[0][:6, 0, :] = torch.arange(6, dtype=torch.float32)[:, None]
    ag._hist.chunks[0][:6, 1, :] = -torch.arange(6, dtype=torch.float32)[:, None]
    tgt = dec._target_tensor(None, None)
    assert tuple(tgt.shape) == (1, 2, ag._Bp) and (tgt[0, 0] == 2).all() and (tgt[0, 1] == -2).all()
    dec.window = 2
    tgt = dec._target_tensor(None, None)
    assert tuple(tgt.shape) == (3, 2, ag._Bp) and tgt[:, 0, 0].tolist() == [1.0, 3.0, 5.0]


# ---- the walk over chunks --------------------------------------------------------------------------------------------------
def rows_of(pieces, filled):
    """global rows of every history per piece, from the (chunk, row) firsts"""
    starts = [np.concatenate(([0], np.cumsum(f)[:-1])) for f in filled]
    return [[int(starts[h][c]) + r + np.arange(length) for h, (c, r) in enumerate(first)] for first, length, _ in pieces]


@pytest.mark.parametrize("window", [1, 3, 5, 255])
def test_window_bookkeeping_across_chunk_boundaries(window):
    from ratinabox_amd._bayes_decoder import window_centre_rows, window_pieces
    filled = [[37, 60, 150, 53 + 300], [400, 200], [7] * 85 + [5]]
    for start, stop in ((0, 600), (11, 598), (36, 38), (590, 600), (100, 100)):
        n_windows, pieces = window_pieces(filled, start, stop, window, max_rows=97)
        assert n_windows == (stop - start) // window
        end = start + n_windows * window
        seen = []
        for (first, length, row0), rows in zip(pieces, rows_of(pieces, filled)):
            assert 1 <= length <= 97 and all(np.array_equal(r, rows[0]) for r in rows)     # the same steps of every history
            assert row0 == rows[0][0] - start
            for h, (c, r) in enumerate(first):
                assert r + length <= filled[h][c]                                          # inside ONE chunk of each
            w = orc.window_of_rows(row0, length, window, n_windows)
            assert (w >= 0).all() and np.array_equal(w, (rows[0] - start) // window)
            seen.extend(rows[0].tolist())
        assert seen == list(range(start, end))                                             # every row once, leftovers dropped
        centres = window_centre_rows(start, n_windows, window)
        assert centres.dtype == np.int64 and centres.tolist() == [start + w * window + window // 2 for w in range(n_windows)]
        assert n_windows == 0 or (centres[-1] < end and centres[0] >= start)
    with pytest.raises(ValueError, match="window"):
        window_pieces(filled, 0, 600, 0)
    with pytest.raises(ValueError, match="window"):
        window_pieces(filled, 0, 600, 256)
