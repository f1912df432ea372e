"""No-GPU checks of the Gaussian-process decoder: the tests' float64 oracle (tests/gp_decoder_oracle.py) and
GPDecoder.from_samples on host tensors against scikit-learn's recorded GaussianProcessRegressor on the reference's decoding
scenario (tests/golden/gp_decoder_reference.npz), the rule that chooses the training samples, the class-level refusals, the
ABI of riab_gp_predict with every refusal produced by validation alone, and the fp32 emulation of the kernel's arithmetic
that the GPU allowance (tests/test_gpu_gp_decoder.py) rests on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import gp_decoder_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "riab_hip.h")
SCENARIO = os.path.join(ROOT, "tests", "golden", "decoder_reference.npz")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gp_decoder_reference.npz")
COLUMNS = {"pc": slice(0, 20), "gc": slice(20, 40), "all": slice(0, 40)}
PRED_ALLOWANCE = 1e-12   # metres: two float64 solutions of a system of cond 1.4e4, predictions of size 1


@pytest.fixture(scope="module")
def S():
    return dict(np.load(SCENARIO))


@pytest.fixture(scope="module")
def G():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def L():
    from ratinabox_amd import _lib
    return _lib


def scenario(S, G, tag):
    """(X (480, n), y (480, 2), the 600 test rows (600, n), length scale, alpha) of one tag, float64"""
    n_train, stride = int(S["n_train"]), int(S["stride"])
    fr, pos = S["fr"][:, COLUMNS[tag]].astype(np.float64), S["pos"].astype(np.float64)
    return fr[:n_train:stride], pos[:n_train:stride], fr[n_train:], float(G[f"length_scale_{tag}"]), float(G["alpha"])


def alpha_allowance(X, ell, alpha, want):
    """64 cond(K + alpha I) 2^-53 max|alpha_|, the condition number computed here"""
    cond = np.linalg.cond(orc.gram(X, ell, alpha))
    return 64.0 * cond * 2.0 ** -53 * np.abs(want).max(), cond


def test_golden_is_the_reference_setup(S, G):
    assert float(G["alpha"]) == 0.01
    for tag, cols in COLUMNS.items():
        n = cols.stop - cols.start
        assert G[f"alpha_{tag}"].shape == (480, 2) and G[f"pred_{tag}"].shape == (600, 2)
        assert float(G[f"length_scale_{tag}"]) == np.sqrt(n / 20)
    assert len(range(0, int(S["n_train"]), int(S["stride"]))) == 480 and len(S["pos"]) - int(S["n_train"]) == 600


@pytest.mark.parametrize("tag", list(COLUMNS))
def test_oracle_reproduces_sklearn(S, G, tag):
    """Measured here: predictions within 1.2e-14 (pc), 2.1e-14 (gc), 4.4e-15 m (all); alpha_ within 2.4e-13, 1.6e-13, 3.3e-13
    against allowances of 4.8e-10, 1.6e-9, 1.2e-10 (cond 1.4e4, 1.5e4, 1.3e4)."""
    X, y, Xq, ell, alpha = scenario(S, G, tag)
    got = orc.fit(X, y, ell, alpha)
    allow, cond = alpha_allowance(X, ell, alpha, G[f"alpha_{tag}"])
    err_a = np.abs(got - G[f"alpha_{tag}"]).max()
    err_p = np.abs(orc.predict(Xq, X, got, ell) - G[f"pred_{tag}"]).max()
    print(f"{tag}: oracle against sklearn: alpha_ {err_a:.3g} (allowance {allow:.3g}, cond {cond:.3g}), predictions {err_p:.3g} m")
    assert err_a <= allow and err_p <= PRED_ALLOWANCE


@pytest.mark.parametrize("tag", list(COLUMNS))
def test_from_samples_on_host_tensors(S, G, tag):
    """Measured here: alpha_ within 6.2e-13 (pc), 3.3e-12 (gc), 3.6e-13 (all); predictions within 1.7e-14, 4.4e-14, 5.1e-15 m."""
    import torch
    from ratinabox_amd import GPDecoder
    X, y, Xq, ell, alpha = scenario(S, G, tag)
    dec = GPDecoder.from_samples(torch.from_numpy(X), torch.from_numpy(y), ell, alpha)
    assert dec.alpha_.dtype == torch.float64 and tuple(dec.alpha_.shape) == (480, 2) and dec.alpha_.device.type == "cpu"
    assert dec.X_train_.data_ptr() == torch.from_numpy(X).data_ptr() and dec.n_samples == 480 and dec.n_dropped == 0
    assert dec.length_scale == ell and dec.alpha == alpha and dec.target == "pos"
    assert dec.train_rows is None and dec.train_agents is None and not hasattr(dec, "as_layer")
    allow, _ = alpha_allowance(X, ell, alpha, G[f"alpha_{tag}"])
    err_a = np.abs(dec.alpha_.numpy() - G[f"alpha_{tag}"]).max()
    err_p = np.abs(dec.mean_float64(torch.from_numpy(Xq)).numpy() - G[f"pred_{tag}"]).max()
    print(f"{tag}: from_samples against sklearn: alpha_ {err_a:.3g} (allowance {allow:.3g}), predictions {err_p:.3g} m")
    assert err_a <= allow and err_p <= PRED_ALLOWANCE
    # length_scale=None is the reference's rule sqrt(n / 20)
    assert GPDecoder.from_samples(torch.from_numpy(X[:8]), torch.from_numpy(y[:8])).length_scale == np.sqrt(X.shape[1] / 20)


def test_from_samples_refusals():
    import torch
    from ratinabox_amd import GPDecoder
    rng = np.random.RandomState(0)
    X, y = torch.from_numpy(rng.rand(6, 3)), torch.from_numpy(rng.rand(6, 2))
    with pytest.raises(ValueError, match="alpha"):
        GPDecoder.from_samples(X, y, 1.0, alpha=-0.1)
    for bad in ([1.0, 2.0, 3.0], np.ones(3), (1.0,)):
        with pytest.raises(ValueError, match="scalar"):
            GPDecoder.from_samples(X, y, bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="length_scale"):
            GPDecoder.from_samples(X, y, bad)
    with pytest.raises(ValueError, match="float64"):
        GPDecoder.from_samples(X.float(), y)
    with pytest.raises(ValueError, match="float64"):
        GPDecoder.from_samples(X, y[:5])
    with pytest.raises(ValueError, match="target columns"):
        GPDecoder.from_samples(X, torch.zeros(6, 5, dtype=torch.float64))
    Xn = X.clone()
    Xn[2, 1] = float("nan")
    with pytest.raises(ValueError, match="rate is not finite"):
        GPDecoder.from_samples(Xn, y)
    # duplicate samples and no regulariser: the factorisation fails and the message names alpha
    with pytest.raises(ValueError, match="alpha"):
        GPDecoder.from_samples(torch.cat([X, X]), torch.cat([y, y]), 1.0, alpha=0.0)
    bare = GPDecoder.from_samples(X, y, 1.0)
    with pytest.raises(ValueError, match="no populations"):
        bare.decode_tensor()
    with pytest.raises(ValueError, match="widths"):
        bare.predict_tensor([torch.zeros(1, 2, 4), torch.zeros(1, 1, 4)])


def test_selection_rule():
    from ratinabox_amd._gp_decoder import select_samples
    # everything fits: every candidate, time-major
    for R, B, N in ((480, 1, 4096), (7, 3, 21), (7, 3, 100), (1, 5, 5)):
        rows, agents = select_samples(R, B, N)
        assert np.array_equal(rows, np.repeat(np.arange(R), B)) and np.array_equal(agents, np.tile(np.arange(B), R))
        assert rows.dtype == agents.dtype == np.int64
    # more candidates than samples: sorted, unique, in range, no more than max_samples, and the oracle's choice
    for R, B, N in ((64, 16, 256), (120, 10, 512), (1000, 1024, 4096), (300, 1, 50), (7, 3, 20), (5000, 2, 16384)):
        rows, agents = select_samples(R, B, N)
        flat = rows * B + agents
        assert len(flat) <= N and (np.diff(flat) > 0).all()
        assert rows.min() >= 0 and rows.max() < R and agents.min() >= 0 and agents.max() < B
        orows, oagents = orc.select_samples(R, B, N)
        assert np.array_equal(rows, orows) and np.array_equal(agents, oagents)
    # R a multiple of B, R B / max_samples = 4 a divisor of B: a stride over the flattened index (0, 4, 8, ... = agents
    # 0, 4, 8, 12 only) would leave 12 of the 16 agents without a sample.  The equal share is 16 of 256; the oracle's rule
    # gives every agent 15..17 (checked below on the oracle).  Cap, asserted on the package's own result: twice the equal
    # share; floor: half of it.
    rows, agents = select_samples(64, 16, 256)
    counts = np.bincount(agents, minlength=16)
    print("samples per agent at R = 64, B = 16, max_samples = 256:", counts.tolist())
    assert len(rows) == 256 and counts.max() <= 32 and counts.min() >= 8
    ocounts = np.bincount(orc.select_samples(64, 16, 256)[1], minlength=16)
    assert ocounts.max() == 17 and ocounts.min() == 15
    assert np.array_equal(np.bincount(rows, minlength=64), np.full(64, 4))   # every row is used, 4 samples each


def test_class_level_refusals_on_cpu_objects():
    """Every refusal is raised before any native call: the objects live on device="cpu", where no kernel can run."""
    import ratinabox_amd as riab
    np.random.seed(0)
    env = riab.Environment({})
    ag = riab.Agent(env, {"n_agents": 8, "device": "cpu"})
    other = riab.Agent(env, {"n_agents": 8, "device": "cpu"})
    pcs = riab.PlaceCells(ag, {"n": 4})
    gcs = riab.GridCells(ag, {"n": 3})
    foreign = riab.PlaceCells(other, {"n": 4})
    for bad in (0, -1, 16385, 2.5):
        with pytest.raises(ValueError, match="max_samples"):
            riab.fit_gp_decoder([pcs], max_samples=bad)
    with pytest.raises(ValueError, match="scalar"):
        riab.fit_gp_decoder([pcs], length_scale=[0.3, 0.4, 0.5, 0.6])
    with pytest.raises(ValueError, match="alpha"):
        riab.fit_gp_decoder([pcs], alpha=-0.5)
    with pytest.raises(ValueError, match="stride"):
        riab.fit_gp_decoder([pcs], stride=0)
    with pytest.raises(ValueError, match="target"):
        riab.fit_gp_decoder([pcs], target="speed")
    # ... and the population and row errors shared with the linear decoder
    with pytest.raises(ValueError, match="one Agent"):
        riab.fit_gp_decoder([pcs, foreign])
    with pytest.raises(ValueError, match="1..8 populations"):
        riab.fit_gp_decoder([pcs] * 9)
    with pytest.raises(ValueError, match="1..8 populations"):
        riab.fit_gp_decoder([])
    with pytest.raises(ValueError, match="no recorded rates"):
        riab.fit_gp_decoder([pcs, gcs])
    with pytest.raises(ValueError, match="no recorded rates"):
        pcs.fit_gp_decoder()
    ag._hist.reserve(5)
    ag._times = [0.1 * (i + 1) for i in range(5)]
    pcs._hist_fr.reserve(3)
    gcs._hist_fr.reserve(5)
    with pytest.raises(ValueError, match="every population's rates at every row"):
        riab.fit_gp_decoder([gcs, pcs])
    with pytest.raises(ValueError, match="every population's rates at every row"):
        pcs.fit_gp_decoder(t_start=0.1, t_end=None)
    with pytest.raises(ValueError, match="samples must index"):
        gcs.fit_gp_decoder(samples=([0, 5], [0, 1]))
    with pytest.raises(ValueError, match="samples must index"):
        gcs.fit_gp_decoder(samples=([0, 1], [0, 8]))
    with pytest.raises(ValueError, match="equal length"):
        gcs.fit_gp_decoder(samples=([0, 1, 2], [0, 1]))


def test_symbol_declared_exported_prototyped_documented(L):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\briab_gp_predict\s*\(([^)]*)\)\s*;", src)
    assert m, "riab_gp_predict is not declared in riab_hip.h"
    assert len(m.group(1).split(",")) == 11 == len(L.PROTOTYPES["riab_gp_predict"][1]) and hasattr(L.lib, "riab_gp_predict")
    raw = open(HEADER).read()
    assert int(re.search(r"#define RIAB_ABI_VERSION (\d+)", raw).group(1)) == 11 == L.ABI_VERSION == L.lib.riab_abi_version()
    for name, val in (("RIAB_GP_MAX_TRAIN", L.GP_MAX_TRAIN), ("RIAB_GP_MAX_OUT", L.GP_MAX_OUT)):
        assert int(re.search(rf"#define {name} (\d+)", raw).group(1)) == val
    assert L.GP_MAX_TRAIN == 16384 and L.GP_MAX_OUT == 4
    assert L.lib.riab_abi_sizeof(5) == C.sizeof(L.RiabFFInput)          # (the struct the entry point reuses is unchanged)
    assert "riab_gp_predict" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    from ratinabox_amd import _build
    assert "riab_gp.hip" in _build.SOURCES


def test_argument_errors_before_launch(L):
    """Every refusal of riab_gp_predict is produced by validation alone: no device needed."""
    p, q = 4096, 4096 + 4

    def call(rates=p, wt=p, n_in=3, n_inputs=1, sq=p, alpha=p, D=2, n_train=40, inv=0.5, T=1, B=8, out=p, null_inputs=False):
        arr = (L.RiabFFInput * 9)()
        for a in arr:
            a.rates, a.wt, a.n_in = rates, wt, n_in
        return L.lib.riab_gp_predict(None if null_inputs else arr, n_inputs, sq, alpha, D, n_train, inv, T, B, out, None)
    assert call(T=0) == 0                                                         # nothing to do, nothing launched
    for null in ("rates", "wt", "sq", "alpha", "out"):
        assert call(**{null: None}) == L.EINVAL, null
    assert call(null_inputs=True) == L.EINVAL
    assert call(n_inputs=0) == L.EINVAL and call(n_inputs=9) == L.EINVAL and call(n_inputs=8, T=0) == 0
    assert call(n_in=0) == L.EINVAL and call(n_in=-3) == L.EINVAL
    assert call(D=0) == L.EINVAL and call(D=5) == L.EINVAL and call(D=1, T=0) == 0 and call(D=4, T=0) == 0
    assert call(n_train=0) == L.EINVAL and call(n_train=-1) == L.EINVAL
    assert call(n_train=L.GP_MAX_TRAIN + 1) == L.ETOOBIG and call(n_train=L.GP_MAX_TRAIN, T=0) == 0
    assert call(B=6) == L.EALIGN == -2 and call(B=0) == L.EINVAL and call(T=-1) == L.EINVAL
    for mis in ("rates", "wt", "sq", "alpha", "out"):
        assert call(**{mis: q}) == L.EALIGN, mis
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(inv=bad) == L.EINVAL, bad
    assert call(T=1 << 40) == L.ETOOBIG and call(T=1 << 31, B=8) == L.ETOOBIG
    assert call(T=1 << 62, B=512) == L.ETOOBIG and call(T=1 << 61, B=1024) == L.ETOOBIG    # (T * tiles wraps in 64 bits)


@pytest.mark.parametrize("tag", list(COLUMNS))
def test_fp32_emulation_on_the_golden(S, G, tag):
    """The kernel's arithmetic emulated in float32 against the float64 prediction: worst error <= 2^-24 sum_j |alpha_jd|.
    Measured here: 0.50 (pc), 0.25 (gc), 0.21 (all) of that.  The GPU test allows 8 of it."""
    X, y, Xq, ell, alpha = scenario(S, G, tag)
    a = G[f"alpha_{tag}"]
    ratio = (np.abs(orc.emulate_fp32(Xq, X, a, ell) - G[f"pred_{tag}"]) / (2.0 ** -24 * orc.l1(a))).max()
    print(f"{tag}: fp32 emulation, worst |error| / (2^-24 |alpha|_1) = {ratio:.3g}")
    assert ratio <= 1.0


def test_fp32_emulation_on_synthetic_place_cells():
    """The same at a wide population and at a large training set, on synthetic Gaussian place cells at scattered positions:
    n = 1024 cells with N = 4096 samples, n = 20 cells with N = 8192.  The coefficients come from `orc.fit_large` (the Gram
    matrix in the GEMM form: any coefficients serve, both sides of the comparison use the same ones); the float64 side of the
    comparison is the oracle's direct-difference prediction.  Measured here: 0.21 and 0.50."""
    rng = np.random.RandomState(2)
    for n, N in ((1024, 4096), (20, 8192)):
        centres = rng.rand(n, 2)
        pos, posq = rng.rand(N, 2), rng.rand(64, 2)
        rates = lambda p: np.exp(-((p[:, None, :] - centres[None]) ** 2).sum(-1) / (2 * 0.2 ** 2)).astype(np.float32).astype(np.float64)
        X, Xq, ell = rates(pos), rates(posq), np.sqrt(n / 20)
        a = orc.fit_large(X, pos, ell, 0.01)
        ratio = (np.abs(orc.emulate_fp32(Xq, X, a, ell) - orc.predict(Xq, X, a, ell)) / (2.0 ** -24 * orc.l1(a))).max()
        print(f"n = {n}, N = {N}: fp32 emulation, worst |error| / (2^-24 |alpha|_1) = {ratio:.3g}")
        assert ratio <= 1.0
