"""The Gaussian-process decoder's predictive variance on the device (riab_gp_predict_var in csrc/riab_gp.hip,
GPDecoder.predict_tensor(return_std=True)) against the float64 restatement (tests/gp_variance_oracle.py) and scikit-learn's
recorded predict(return_std=True) (tests/golden/gp_variance_reference.npz).

The tolerance for var is orc.GPU_VAR_TOLERANCE = 8 * 1.6e-6: the fp32 emulation of the two kernels' arithmetic stays within
1.6e-6 of the float64 variance on the golden cases and at N = 512 (tests/test_gp_variance_cpu.py::test_fp32_budget); the
factor 8 is the margin for v_exp_f32 and the kernels' summation order.  The std is compared through var = std^2 (the
derivative of the square root is unbounded at 0).

Shapes: Np = 32 (one 32-sample block per step, MT = 1), 96 (N = 70 ragged, MT = 2) and 160 (N = 130: MT = 4, two blocks, the
second ragged); B = 8 with 5 real columns and B = 132 with 130 (a second position tile with two live columns); T = 1 and
3; one and two populations."""
import os

import numpy as np
import pytest
import torch

from tests import gp_variance_oracle as orc
from tests.guard_arena import CANARIES, GuardArena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gp_variance_reference.npz")
DEV = "cuda"
HUGE = np.float32(3.0e38)
TOL = orc.GPU_VAR_TOLERANCE

# (N, widths, length scale): Np = 32, 96, 160
MODELS = {"n20": (20, (9,), 0.5), "n70": (70, (7, 50), 1.2), "n130": (130, (17,), 0.7), "n130x2": (130, (7, 50), 1.2)}
# (model, B, n_real, T)
CASES = [("n20", 8, 5, 1), ("n20", 132, 130, 3), ("n70", 8, 5, 3), ("n70", 132, 130, 1), ("n130", 8, 5, 1),
         ("n130", 132, 130, 3), ("n130x2", 132, 130, 1)]
_CACHE = {}


@pytest.fixture(scope="module")
def riab():
    import ratinabox_amd
    return ratinabox_amd


def model(riab, name, alpha=0.01):
    """(decoder fitted on the device from bare samples, X float64 (N, n), length scale, alpha), made once"""
    key = (name, alpha)
    if key not in _CACHE:
        N, widths, ell = MODELS[name]
        rng = np.random.RandomState(7 + N + len(widths))
        X = (rng.rand(N, sum(widths)) ** 3).astype(np.float32).astype(np.float64)
        y = rng.rand(N, 2)
        dec = riab.GPDecoder.from_samples(torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV), ell, alpha, widths=list(widths))
        _CACHE[key] = (dec, X, ell, alpha)
    return _CACHE[key]


def queries(name, B, n_real, T, seed=3):
    """(T, B, n) float32: training points, points near them, random points and points far outside in turn (so that five
    columns hold one of each); the padding columns b >= n_real hold NaN"""
    N, widths, ell = MODELS[name]
    n = sum(widths)
    rng = np.random.RandomState(seed + B + T)
    X = (np.random.RandomState(7 + N + len(widths)).rand(N, n) ** 3).astype(np.float32)
    kind = (np.arange(T * B).reshape(T, B) + np.arange(T)[:, None]) % 4
    base = X[rng.randint(0, N, size=(T, B))]
    Q = np.where(kind[..., None] == 0, base,
                 np.where(kind[..., None] == 1, base + 0.6 * ell * rng.randn(T, B, n) / np.sqrt(n),
                          np.where(kind[..., None] == 2, rng.rand(T, B, n) ** 3,
                                   base + 4.0 * ell * np.sign(rng.randn(T, B, n)) / np.sqrt(n)))).astype(np.float32)
    Q[:, n_real:] = np.nan
    return Q


def split(Q, widths):
    """queries (T, B, n) -> the decoder's inputs [(T, n_l, B)] on the device"""
    out, k = [], 0
    for w in widths:
        out.append(torch.from_numpy(np.ascontiguousarray(Q[:, :, k:k + w].transpose(0, 2, 1))).to(DEV))
        k += w
    return out


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name, B, n_real, T", CASES)
def test_parity_with_the_float64_oracle(riab, name, B, n_real, T):
    dec, X, ell, alpha = model(riab, name)
    Q = queries(name, B, n_real, T)
    rates = split(Q, dec.widths)
    mean, std = dec.predict_tensor(rates, return_std=True)
    assert tuple(mean.shape) == (T, 2, B) and tuple(std.shape) == (T, B) and std.dtype == mean.dtype == torch.float32
    want = np.maximum(orc.variance(Q[:, :n_real].reshape(T * n_real, -1).astype(np.float64), X, ell, alpha), 0.0).reshape(T, n_real)
    got = std.cpu().numpy()[:, :n_real].astype(np.float64) ** 2
    err = float(np.abs(got - want).max())
    print(f"{name} B {B} T {T}: max |var - float64 var| = {err:.3g} (tolerance {TOL:.3g}); var in [{want.min():.3g}, {want.max():.3g}]")
    assert want.min() <= 0.05 and want.max() >= 0.9          # (the case exercises the variance)
    assert np.isfinite(got).all() and (got >= 0).all() and err <= TOL
    assert np.array_equal(bits(mean), bits(dec.predict_tensor(rates)))                 # the mean's bits, padding included
    # the float64 definition in the package agrees with the oracle on a handful of samples
    s64 = dec.std_float64(torch.from_numpy(Q[0, :4].astype(np.float64)).to(DEV)).cpu().numpy()
    assert np.abs(s64 ** 2 - want[0, :4]).max() <= 1e-10


@pytest.mark.parametrize("c", ["a", "b", "c"])
def test_golden_cases_against_sklearn(riab, c):
    G = dict(np.load(GOLDEN))
    X, y, Xq = G[f"X_{c}"], G[f"y_{c}"], G[f"Xq_{c}"]
    dec = riab.GPDecoder.from_samples(torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV), float(G[f"length_scale_{c}"]),
                                      float(G["alpha"]), widths=[int(w) for w in G[f"widths_{c}"]])
    S = len(Xq)
    B = (S + 3) // 4 * 4 + 4
    Q = np.full((1, B, Xq.shape[1]), np.nan, dtype=np.float32)
    Q[0, :S] = Xq
    mean, std = dec.predict_tensor(split(Q, dec.widths), return_std=True)
    got = std.cpu().numpy()[0, :S].astype(np.float64) ** 2
    err = float(np.abs(got - G[f"y_std_{c}"] ** 2).max())
    lml = abs(dec.log_marginal_likelihood_ - float(G[f"lml_{c}"])) / abs(float(G[f"lml_{c}"]))
    print(f"{c}: max |var - sklearn's y_std^2| = {err:.3g} (tolerance {TOL:.3g}); lml relative {lml:.3g}")
    assert err <= TOL and lml <= 1e-9
    assert np.array_equal(bits(mean), bits(dec.predict_tensor(split(Q, dec.widths))))


def test_determinism_over_rows_columns_and_workspaces(riab):
    """A row alone against the row inside T = 3; B = 132 against its two column blocks; every cut of the workspace against
    one piece: the same bits."""
    for name in ("n70", "n130"):
        dec, X, ell, alpha = model(riab, name)
        Np = (dec.n_samples + 31) // 32 * 32
        Q = queries(name, 132, 130, 3)
        rates = split(Q, dec.widths)
        mean, std = dec.predict_tensor(rates, return_std=True)
        for t in range(3):
            m1, s1 = dec.predict_tensor([x[t:t + 1] for x in rates], return_std=True)
            assert np.array_equal(bits(m1[0]), bits(mean[t])) and np.array_equal(bits(s1[0]), bits(std[t]))
        for c0, c1 in ((0, 128), (128, 132)):
            m2, s2 = dec.predict_tensor([x[:, :, c0:c1].contiguous() for x in rates], return_std=True)
            assert np.array_equal(bits(m2), bits(mean[:, :, c0:c1])) and np.array_equal(bits(s2), bits(std[:, c0:c1]))
        for limit in (4 * Np * 132 * 2, 4 * Np * 132, 4 * Np * 132 - 1, 4 * Np * 128):   # 2 + 1 rows; a row each; column blocks
            m3, s3 = dec.predict_tensor(rates, return_std=True, max_workspace_bytes=limit)
            assert np.array_equal(bits(m3), bits(mean)) and np.array_equal(bits(s3), bits(std)), limit
        with pytest.raises(ValueError, match="max_workspace_bytes"):
            dec.predict_tensor(rates, return_std=True, max_workspace_bytes=4 * Np * 128 - 1)


def test_decode_tensor_over_a_chunked_history(riab):
    """decode_tensor(return_std=True) walks the history chunk by chunk: the bits of predict_tensor on the stacked rows."""
    np.random.seed(5)
    ag = riab.Agent(riab.Environment({}), {"n_agents": 10, "dt": 0.05, "seed": 21})
    pcs, gcs = riab.PlaceCells(ag, {"n": 33, "widths": 0.3}), riab.GridCells(ag, {"n": 20})
    pcs._hist_fr.preallocate(100)

    def loop(k):
        for _ in range(k):
            ag.update()
            pcs.update()
            gcs.update()
    ag.simulate(17)
    loop(20)
    ag.simulate(23)
    assert len(ag.history["t"]) == 60 and list(np.cumsum(ag._hist.filled)) != list(np.cumsum(pcs._hist_fr.filled))
    t = np.asarray(ag.history["t"])
    dec = riab.fit_gp_decoder([pcs, gcs], t_end=t[40], max_samples=130)
    assert 96 < dec.n_samples <= 130 and isinstance(dec.log_marginal_likelihood_, float)
    plain = dec.decode_tensor(t_start=t[40])
    assert dec._linv_t is None                                     # (no variance table without return_std)
    mean, std = dec.decode_tensor(t_start=t[40], return_std=True)
    assert tuple(mean.shape) == (20, 2, 12) and tuple(std.shape) == (20, 12) and torch.equal(mean, plain)
    rows = [p.get_history_tensors()[0][40:].contiguous() for p in (pcs, gcs)]
    m2, s2 = dec.predict_tensor(rows, return_std=True)
    assert np.array_equal(bits(mean), bits(m2)) and np.array_equal(bits(std), bits(s2))
    m3, s3 = dec.decode_tensor(t_start=t[40], return_std=True, max_workspace_bytes=4 * 160 * 12)
    assert np.array_equal(bits(mean), bits(m3)) and np.array_equal(bits(std), bits(s3))
    dm, ds = dec.decode(t_start=t[40], return_std=True)
    assert dm.shape == (20, 10, 2) and ds.shape == (20, 10) and np.array_equal(dm, dec.decode(t_start=t[40]))
    assert np.array_equal(ds, std.cpu().numpy()[:, :10]) and np.isfinite(ds).all() and (ds >= 0).all() and (ds <= 1).all()


def abi_call(L, dec, rates, linv_t, ws, var, mean):
    wts, sq, al = dec._device_tables(rates[0].device)
    arr = (L.RiabFFInput * len(rates))()
    for a, x, w in zip(arr, rates, wts):
        a.rates, a.wt, a.n_in = x.data_ptr(), w.data_ptr(), int(x.shape[1])
    T, B = int(rates[0].shape[0]), int(rates[0].shape[2])
    rc = L.lib.riab_gp_predict_var(arr, len(rates), L.ptr(sq), L.ptr(al), int(al.shape[0]), dec.n_samples,
                                   1.0 / (2.0 * dec.length_scale ** 2), L.ptr(linv_t), T, B, L.ptr(ws), L.ptr(var),
                                   None if mean is None else L.ptr(mean), L.current_stream())
    assert rc == 0
    torch.cuda.synchronize()


def test_triangular_half_is_skipped_not_masked(riab):
    """Np = 256 (MT = 4): for the columns i < 128 of linv_t the rows j >= 128 are never read.  Filled with NaN they change
    no bit; the part above the diagonal that IS read is zero in both tables."""
    from ratinabox_amd import _lib as L
    N, n = 250, 12
    rng = np.random.RandomState(12)
    X = (rng.rand(N, n) ** 3).astype(np.float32).astype(np.float64)
    dec = riab.GPDecoder.from_samples(torch.from_numpy(X).to(DEV), torch.from_numpy(rng.rand(N, 1)).to(DEV), 0.6, 0.01)
    clean = dec._variance_table(torch.empty(0, device=DEV).device)
    assert tuple(clean.shape) == (256, 256) and not clean.tril(-1).any()
    dirty = clean.clone()
    dirty[128:, :128] = float("nan")
    Q = (rng.rand(2, 132, n) ** 3).astype(np.float32)
    Q[:, :40] = X[:40]
    rates = split(Q, [n])
    out = []
    for table in (clean, dirty):
        ws = torch.empty((2, 256, 132), dtype=torch.float32, device=DEV)
        var = torch.full((2, 132), -1.0, dtype=torch.float32, device=DEV)
        abi_call(L, dec, rates, table, ws, var, None)
        out.append(var)
    assert torch.isfinite(out[0]).all() and (out[0] >= 0).all() and float(out[0].max()) > 0.5 and float(out[0].min()) < 0.05
    assert np.array_equal(bits(out[0]), bits(out[1]))
    want = np.maximum(orc.variance(Q.reshape(-1, n).astype(np.float64), X, 0.6, 0.01), 0.0).reshape(2, 132)
    assert np.abs(out[0].cpu().numpy() - want).max() <= TOL


@pytest.mark.parametrize("name", ["n70", "n130"])
def test_poisoned_columns_and_padding(riab, name):
    dec, X, ell, alpha = model(riab, name)
    B, n_real, T = 132, 130, 3
    Q = queries(name, B, n_real, T)
    clean = Q.copy()
    clean[:, n_real:] = 0.25
    base_m, base_s = dec.predict_tensor(split(clean, dec.widths), return_std=True)
    n = Q.shape[2]
    for poison in (np.float32(np.nan), np.float32(np.inf), HUGE):
        Qp = Q.copy()
        Qp[:, n_real:] = poison                                          # padding columns: nobody else's business
        m, s = dec.predict_tensor(split(Qp, dec.widths), return_std=True)
        assert np.array_equal(bits(s[:, :n_real]), bits(base_s[:, :n_real]))
        assert np.array_equal(bits(m[:, :, :n_real]), bits(base_m[:, :, :n_real]))
        for t, b, k in ((0, 0, 0), (T - 1, 129, n - 1), (1, 64, n // 2)):
            Qp[t, b, k] = poison
        m, s = dec.predict_tensor(split(Qp, dec.widths), return_std=True)
        keep = np.ones((T, B), dtype=bool)
        keep[:, n_real:] = False
        for t, b in ((0, 0), (T - 1, 129), (1, 64)):
            assert torch.isnan(s[t, b]) and not torch.isfinite(m[t, :, b]).any()
            keep[t, b] = False
        assert np.array_equal(bits(s)[keep], bits(base_s)[keep])
        assert np.array_equal(bits(m).transpose(0, 2, 1)[keep], bits(base_m).transpose(0, 2, 1)[keep])


def test_clamp_at_a_training_point(riab):
    """alpha = 1e-6, queries equal to training points: the float64 variance is ~1e-6 and the fp32 sum of squares can pass 1;
    var is clamped at 0, never negative and never NaN."""
    dec, X, ell, alpha = model(riab, "n70", alpha=1e-6)
    Q = np.zeros((1, 72, X.shape[1]), dtype=np.float32)
    Q[0, :70] = X
    Q[0, 70:] = X[:2]
    mean, std = dec.predict_tensor(split(Q, dec.widths), return_std=True)
    s = std.cpu().numpy()
    print(f"alpha = 1e-6 at the training points: std in [{s.min():.3g}, {s.max():.3g}], {int((s == 0).sum())} of {s.size} clamped")
    assert np.isfinite(s).all() and (s >= 0).all() and s.max() <= 0.05


@pytest.mark.parametrize("name, B, n_real, T, with_mean", [("n70", 8, 5, 3, True), ("n130", 132, 130, 1, True),
                                                          ("n130x2", 8, 5, 1, False), ("n20", 132, 130, 3, False)])
def test_guard_bands(riab, name, B, n_real, T, with_mean):
    """out_var, out_mean and the workspace inside canary-filled arenas: nothing outside them is written, every word of them
    is (the padded rows of the workspace and the padding columns included), and the results do not depend on what the
    memory held.  With out_mean null the other two are written the same."""
    from ratinabox_amd import _lib as L
    dec, X, ell, alpha = model(riab, name)
    Np = (dec.n_samples + 31) // 32 * 32
    Q = queries(name, B, n_real, T)
    Q[:, n_real:] = 0.5                                                  # (finite padding: every output word is comparable)
    rates = split(Q, dec.widths)
    linv_t = dec._variance_table(rates[0].device)
    wts, sq, al = dec._device_tables(rates[0].device)
    ref_v, ref_m = torch.ops.riab.gp_predict_var(rates, wts, sq, al, linv_t, dec.n_samples, 1.0 / (2.0 * ell ** 2),
                                                 torch.empty(T * Np * B, dtype=torch.float32, device=DEV), True)
    seen = [None, None, None]
    for canary in CANARIES:
        arena = GuardArena(canary)
        var = arena.view((T, B), torch.float32, DEV)
        ws = arena.view((T, Np, B), torch.float32, DEV)
        mean = arena.view((T, 2, B), torch.float32, DEV) if with_mean else None
        abi_call(L, dec, rates, linv_t, ws, var, mean)
        seen[0] = arena.check(var, other=seen[0])
        seen[1] = arena.check(ws, other=seen[1])
        if with_mean:
            seen[2] = arena.check(mean, other=seen[2])
            assert np.array_equal(seen[2].view(np.uint32), bits(ref_m))
        assert np.array_equal(seen[0].view(np.uint32), bits(ref_v))
        assert np.isfinite(seen[1]).all() and (seen[1] >= 0).all() and (seen[1] <= 1).all()


def test_capture_and_replay(riab):
    """One predict_tensor(return_std=True) captured in a graph (the tables were built by the eager call before it) and
    replayed twice: the eager call's bits both times."""
    dec, X, ell, alpha = model(riab, "n130")
    rates = split(queries("n130", 132, 130, 3), dec.widths)
    eager_m, eager_s = dec.predict_tensor(rates, return_std=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            m, s = dec.predict_tensor(rates, return_std=True)
    torch.cuda.synchronize()
    for _ in range(2):
        m.fill_(-3.0)
        s.fill_(-3.0)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(m), bits(eager_m)) and np.array_equal(bits(s), bits(eager_s))
