"""No-GPU checks of the linear decoder: the tests' float64 oracle against sklearn's recorded results on the reference's
decoding scenario, LinearDecoder.from_moments on host tensors by its backward error, the chunk / stride / piece walker,
the ABI of the riab_history_moments entry points and the class-level refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import decoder_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "riab_hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "decoder_reference.npz")
NEW_SYMBOLS = {"riab_history_moments_workspace": 4, "riab_history_moments": 13}
COLUMNS = {"pc": slice(0, 20), "gc": slice(20, 40), "all": slice(0, 40)}


@pytest.fixture(scope="module")
def G():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def L():
    from ratinabox_amd import _lib
    return _lib


def fixture_rows(G, cols):
    """The fixture as history rows of one agent (B = 4, lane 0 real): (rates (T, n, 4), traj (T, 8, 4)) float32; the
    padding lanes hold NaN rates and 3e38 positions."""
    T = len(G["pos"])
    traj = np.full((T, 8, 4), 3e38, dtype=np.float32)
    traj[:, 0, 0], traj[:, 1, 0] = G["pos"][:, 0], G["pos"][:, 1]
    fr = G["fr"][:, cols]
    rows = np.full((T, fr.shape[1], 4), np.nan, dtype=np.float32)
    rows[:, :, 0] = fr
    return rows, traj


def test_oracle_reproduces_sklearn_on_the_reference_scenario(G):
    """Moments of every 5th training row -> the ridge solve -> predictions on the test rows, against
    sklearn.linear_model.Ridge(alpha=0.01).predict as recorded from the reference's scenario.  Allowance 1e-7 m (two
    float64 solutions of a system of cond 1e6); measured on this fixture: pc 1.2e-13 m, gc 1.3e-14 m, all 1.2e-13 m."""
    n_train, stride, alpha = int(G["n_train"]), int(G["stride"]), float(G["alpha"])
    for tag, cols in COLUMNS.items():
        rows, traj = fixture_rows(G, cols)
        M, dropped = orc.moments([rows[:n_train]], traj[:n_train], (0, 1), 1, stride)
        n = rows.shape[1]
        assert dropped == 0 and M[-1, -1] == len(range(0, n_train, stride)) and M.shape == (n + 3, n + 3)
        coef, icpt = orc.ridge(M, n, 2, alpha)
        pred = orc.predict(coef, icpt, G["fr"][n_train:, cols])
        err = np.abs(pred - G[f"pred_{tag}"]).max()
        print(f"{tag}: oracle against sklearn's predictions: {err:.3g} m")
        assert err <= 1e-7


def test_from_moments_on_host_tensors_by_backward_error(G):
    import torch
    from ratinabox_amd._decoder import LinearDecoder, MomentLayout
    n_train, stride = int(G["n_train"]), int(G["stride"])
    for tag, cols in COLUMNS.items():
        rows, traj = fixture_rows(G, cols)
        M, _ = orc.moments([rows[:n_train]], traj[:n_train], (0, 1), 1, stride)
        n = rows.shape[1]
        dec = LinearDecoder.from_moments(torch.from_numpy(M), MomentLayout([n], "pos"), alpha=0.01)
        assert dec.coef_.dtype == torch.float64 and tuple(dec.coef_.shape) == (2, n) and tuple(dec.intercept_.shape) == (2,)
        assert dec.n_samples == len(range(0, n_train, stride)) and dec.n_dropped == 0 and dec.alpha == 0.01
        assert dec.target == "pos" and dec.moments.data_ptr() == torch.from_numpy(M).data_ptr()
        A, Cc, _, _, _ = orc.centred(M, n, 2)
        A = A + 0.01 * np.eye(n)
        W = dec.coef_.numpy().T
        resid = np.linalg.norm(A @ W - Cc)
        bound = 1e-12 * (np.linalg.norm(A) * np.linalg.norm(W) + np.linalg.norm(Cc))
        print(f"{tag}: backward error {resid:.3g} (bound {bound:.3g})")
        assert resid <= bound
        coef, icpt = orc.ridge(M, n, 2, 0.01)
        x = G["fr"][n_train:, cols]
        diff = np.abs(orc.predict(dec.coef_.numpy(), dec.intercept_.numpy(), x) - orc.predict(coef, icpt, x)).max()
        print(f"{tag}: predictions against the oracle's: {diff:.3g} m")
        assert diff <= 1e-9
    with pytest.raises(ValueError, match="alpha"):
        LinearDecoder.from_moments(torch.from_numpy(M), MomentLayout([n], "pos"), alpha=-1.0)
    with pytest.raises(ValueError, match="moments"):
        LinearDecoder.from_moments(torch.from_numpy(M), MomentLayout([n + 1], "pos"))
    with pytest.raises(ValueError, match="no sample"):
        LinearDecoder.from_moments(torch.zeros_like(torch.from_numpy(M)), MomentLayout([n], "pos"))


def random_chunking(rng, total):
    f = []
    while sum(f) < total:
        f.append(int(rng.randint(0, 9)) if rng.rand() < 0.8 else int(rng.randint(9, 40)))
    return f + [int(rng.randint(0, 5))]   # (histories may be longer than the rows asked for)


def test_history_pieces_random_chunkings():
    from ratinabox_amd._decoder import history_pieces
    rng = np.random.RandomState(3)
    for trial in range(300):
        total = int(rng.randint(1, 90))
        filled = [random_chunking(rng, total) for _ in range(int(rng.randint(1, 5)))]
        start = int(rng.randint(0, total + 1))
        stop = int(rng.randint(start, total + 1))
        stride = int(rng.choice([1, 1, 2, 3, 5, 7, 50]))
        max_rows = None if trial % 3 else int(rng.choice([1, 2, 4, 11]))
        got = []
        for first, length in history_pieces(filled, start, stop, stride, max_rows):
            assert length >= 1 and len(first) == len(filled) and (max_rows is None or length <= max_rows)
            rows0 = {sum(f[:c]) + r for f, (c, r) in zip(filled, first)}
            assert len(rows0) == 1                                     # the same global row in every history
            for f, (c, r) in zip(filled, first):
                assert 0 <= r and r + length <= f[c]                   # inside ONE chunk of each
            g0 = rows0.pop()
            got.extend(range(g0, g0 + length, stride))
        assert got == list(range(start, stop, stride)), (filled, start, stop, stride, max_rows)
    assert history_pieces([[5, 2]], 3, 3) == [] and history_pieces([[5, 2]], 4, 2) == []
    for bad in ((0, 8, 1), (-1, 2, 1), (0, 2, 0)):
        with pytest.raises(ValueError):
            history_pieces([[5, 2], [9]], *bad)


def test_new_symbols_declared_exported_prototyped(L):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, argc in NEW_SYMBOLS.items():
        m = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in riab_hip.h"
        assert len(m.group(1).split(",")) == argc
        assert hasattr(L.lib, name) and len(L.PROTOTYPES[name][1]) == argc
    raw = open(HEADER).read()
    assert int(re.search(r"#define RIAB_ABI_VERSION (\d+)", raw).group(1)) == 11 == L.ABI_VERSION == L.lib.riab_abi_version()
    for name, val in (("RIAB_MOMENTS_MAX_TARGETS", L.MOMENTS_MAX_TARGETS), ("RIAB_MOMENTS_MAX_M", L.MOMENTS_MAX_M)):
        assert int(re.search(rf"#define {name} (\d+)", raw).group(1)) == val
    assert L.lib.riab_abi_sizeof(12) == C.sizeof(L.RiabMomentInput) == 16
    assert "riab_history_moments" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_workspace_is_positive_and_monotone(L):
    ws = L.lib.riab_history_moments_workspace
    for t_step in (1, 2, 5):
        last = 0
        for T in (1, 2, 3, 5, 64, 70, 1000, 4096):
            assert ws(T, t_step, 23, 12) >= max(last, 1)
            last = ws(T, t_step, 23, 12)
        last = 0
        for m in (2, 4, 16, 17, 64, 65, 103, 128, 129, 1027, 4096):
            assert ws(70, t_step, m, 200) >= max(last, 1)
            last = ws(70, t_step, m, 200)
        last = 0
        for B in (4, 12, 64, 68, 200, 4096):
            assert ws(3, t_step, 103, B) >= max(last, 1)
            last = ws(3, t_step, 103, B)
    assert ws(1, 0, 4, 8) == L.EINVAL and ws(1, 1, 0, 8) == L.EINVAL and ws(-1, 1, 4, 8) == L.EINVAL
    assert ws(1, 1, 4, 6) == L.EALIGN and ws(1, 1, L.MOMENTS_MAX_M + 1, 8) == L.ETOOBIG and ws(1 << 40, 1, 4, 8) == L.ETOOBIG


def test_argument_errors_before_launch(L):
    """Every refusal of riab_history_moments is produced by validation alone: no device needed."""
    p, q = 4096, 4096 + 4

    def call(rows=p, n=3, n_inputs=1, traj=p, targets=(0, 1), n_targets=None, T=1, t_step=1, B=8, n_real=8, moments=p,
             dropped=p, ws=p, null_inputs=False, null_targets=False):
        arr = (L.RiabMomentInput * 9)()
        for a in arr:
            a.rows, a.n = rows, n
        tr = (C.c_int32 * 5)(*(list(targets) + [0] * 5)[:5])
        return L.lib.riab_history_moments(None if null_inputs else arr, n_inputs, traj, None if null_targets else tr,
                                          len(targets) if n_targets is None else n_targets, T, t_step, B, n_real, moments,
                                          dropped, ws, None)
    assert call(T=0) == 0                                                         # nothing to do, nothing launched
    for null in ("traj", "moments", "dropped", "ws", "rows"):
        assert call(**{null: None}) == L.EINVAL
    assert call(null_inputs=True) == L.EINVAL and call(null_targets=True) == L.EINVAL
    assert call(B=6, n_real=6) == L.EALIGN == -2
    assert call(rows=q) == L.EALIGN and call(traj=q) == L.EALIGN and call(moments=q) == L.EALIGN and call(ws=q) == L.EALIGN
    assert call(n_inputs=9) == L.EINVAL and call(n_inputs=0) == L.EINVAL and call(n_inputs=8, T=0) == 0
    assert call(n_targets=0) == L.EINVAL and call(n_targets=5) == L.EINVAL and call(targets=(0, 1, 2, 3), T=0) == 0
    assert call(targets=(0, 8)) == L.EINVAL and call(targets=(-1, 1)) == L.EINVAL and call(targets=(7,), T=0) == 0
    assert call(t_step=0) == L.EINVAL and call(t_step=-3) == L.EINVAL
    assert call(n=0) == L.EINVAL and call(n_real=9) == L.EINVAL and call(T=-1) == L.EINVAL
    assert call(T=(1 << 31) // 2, B=8) == L.ETOOBIG and call(T=1 << 40) == L.ETOOBIG    # T * B / 4 >= 2^31 - 1
    assert call(n=L.MOMENTS_MAX_M, T=0) == L.ETOOBIG


def test_class_level_refusals_on_cpu_objects():
    """Every refusal is raised before any native call: the objects live on device="cpu", where no kernel can run."""
    import ratinabox_amd as riab
    from ratinabox_amd import _decoder
    np.random.seed(0)
    env = riab.Environment({})
    ag = riab.Agent(env, {"n_agents": 8, "device": "cpu"})
    other = riab.Agent(env, {"n_agents": 8, "device": "cpu"})
    pcs = riab.PlaceCells(ag, {"n": 4})
    gcs = riab.GridCells(ag, {"n": 3})
    foreign = riab.PlaceCells(other, {"n": 4})
    with pytest.raises(ValueError, match="one Agent"):
        riab.fit_linear_decoder([pcs, foreign])
    with pytest.raises(ValueError, match="no recorded rates"):
        riab.fit_linear_decoder([pcs, gcs])
    with pytest.raises(ValueError, match="no recorded rates"):
        pcs.fit_decoder()
    with pytest.raises(ValueError, match="stride"):
        riab.history_moments_tensor([pcs], stride=0)
    with pytest.raises(ValueError, match="alpha"):
        riab.fit_linear_decoder([pcs], alpha=-0.5)
    with pytest.raises(ValueError, match="target"):
        riab.history_moments_tensor([pcs], target="speed")
    with pytest.raises(ValueError, match="1..8 populations"):
        riab.fit_linear_decoder([pcs] * 9)
    with pytest.raises(ValueError, match="1..8 populations"):
        riab.fit_linear_decoder([])
    with pytest.raises(NotImplementedError, match="spikes"):
        riab.fit_linear_decoder([pcs], spikes=True)
    # histories that do not cover the rows asked for: 5 trajectory rows, 3 of the place cells', 5 of the grid cells'
    ag._hist.reserve(5)
    ag._times = [0.1 * (i + 1) for i in range(5)]
    pcs._hist_fr.reserve(3)
    gcs._hist_fr.reserve(5)
    with pytest.raises(ValueError, match="every population's rates at every row"):
        riab.fit_linear_decoder([gcs, pcs])
    with pytest.raises(ValueError, match="every population's rates at every row"):
        pcs.fit_decoder(t_start=0.1, t_end=None)
    # a decoder built from bare moments has nothing to decode from; layers key inputs by name
    import torch
    M, _ = orc.moments([np.random.rand(6, 4, 4).astype(np.float32)], np.random.rand(6, 8, 4).astype(np.float32), (0, 1), 3)
    bare = _decoder.LinearDecoder.from_moments(torch.from_numpy(M), _decoder.MomentLayout([4], "pos"))
    with pytest.raises(ValueError, match="no populations"):
        bare.decode_tensor()
    twin = riab.PlaceCells(ag, {"n": 4})
    named = _decoder.LinearDecoder.from_moments(torch.from_numpy(orc.moments(
        [np.random.rand(6, 8, 4).astype(np.float32)], np.random.rand(6, 8, 4).astype(np.float32), (0, 1), 3)[0]),
        _decoder.MomentLayout([4, 4], "pos", [pcs, twin]))
    with pytest.raises(ValueError, match="distinct names"):
        named.as_layer()
