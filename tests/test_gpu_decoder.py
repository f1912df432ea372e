"""Linear decoders fitted from the device history (csrc/riab_decoder.hip, ratinabox_amd/_decoder.py) against the float64
restatement (tests/decoder_oracle.py) and sklearn's own results on the reference's decoding scenario
(tests/golden/decoder_reference.npz).

On hand-made samples whose products and sums are exact in float64 in any order (rates k / 32, targets k / 256) the moment
matrix is compared BIT FOR BIT.  On real rates the allowance per element is derived: the products of widened fp32 values
are exact in float64, only the order of the S additions differs, so |dM_ij| <= S * 2^-53 * sum|z_i z_j|."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import decoder_oracle as orc
from tests.guard_arena import CANARIES, GuardArena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "decoder_reference.npz")
DEV = "cuda"
HUGE = np.float32(3.0e38)


@pytest.fixture(scope="module")
def riab():
    import ratinabox_amd
    return ratinabox_amd


@pytest.fixture(scope="module")
def G():
    return dict(np.load(GOLDEN))


def exact_samples(seed, T, widths, B, n_real):
    """(inputs [(T, n_l, B)], traj (T, 8, B)) float32: rates k / 32, trajectory rows k / 256; the padding lanes hold NaN
    rates and 3e38 in every trajectory row."""
    rng = np.random.RandomState(seed)
    inputs = []
    for n in widths:
        x = (rng.randint(0, 32, size=(T, n, B)) / 32.0).astype(np.float32)
        x[:, :, n_real:] = np.nan
        inputs.append(x)
    traj = (rng.randint(0, 256, size=(T, 8, B)) / 256.0).astype(np.float32)
    traj[:, :, n_real:] = HUGE
    return inputs, traj


def run_op(inputs, traj, target_rows, t_step, n_real, pieces=None):
    """torch.ops.riab.history_moments on host arrays: (M, n_dropped) as NumPy / int.  `pieces`: row ranges handed over
    one after the other (each starts on a selected row), accumulating in place."""
    import ratinabox_amd.ops  # noqa: F401  (registers torch.ops.riab.*)
    m = sum(x.shape[1] for x in inputs) + len(target_rows) + 1
    M = torch.zeros((m, m), dtype=torch.float64, device=DEV)
    dropped = torch.zeros(1, dtype=torch.int64, device=DEV)
    dx, dt = [torch.from_numpy(x).to(DEV) for x in inputs], torch.from_numpy(traj).to(DEV)
    for a, b in (pieces or [(0, traj.shape[0])]):
        assert a % t_step == 0
        torch.ops.riab.history_moments([x[a:b] for x in dx], dt[a:b], list(target_rows), t_step, n_real, M, dropped)
    torch.cuda.synchronize()
    return M.cpu().numpy(), int(dropped.item())


# (widths, B, n_real, T, t_step, target rows, pieces): 1, 2 and 3 populations; every n of {1, 15, 16, 17, 33, 100}, so
# that m and each input's first row are ragged against the 16-wide tile and the 64-row block; every B of {4, 12, 64, 68,
# 200} with n_real 1-3 below it; every T of {1, 3, 70}; every t_step of {1, 2, 5}; the rows in 1, 2 and 3 pieces
EXACT_CASES = [
    ((1,), 4, 3, 1, 1, (0, 1), None),
    ((1,), 4, 1, 3, 2, (0, 1), None),
    ((15,), 12, 10, 3, 1, (0, 1), [(0, 1), (1, 3)]),
    ((16,), 64, 63, 1, 5, (2, 3), None),
    ((17,), 68, 65, 3, 5, (4, 5), None),
    ((33,), 200, 197, 70, 5, (0, 1), [(0, 35), (35, 70)]),
    ((100,), 12, 9, 70, 2, (0, 1), [(0, 2), (2, 36), (36, 70)]),
    ((1, 15), 64, 62, 3, 1, (0, 1), [(0, 2), (2, 3)]),
    ((17, 33), 68, 67, 70, 1, (0, 1, 6, 7), [(0, 1), (1, 69), (69, 70)]),
    ((16, 100), 4, 2, 70, 5, (7,), None),
    ((15, 17, 33), 200, 198, 3, 2, (0, 1), None),
    ((100, 1, 16), 12, 11, 70, 1, (0, 1), [(0, 33), (33, 70)]),
    ((33, 100, 17), 68, 66, 1, 1, (1, 0), None),
]


@pytest.mark.parametrize("widths, B, n_real, T, t_step, rows, pieces", EXACT_CASES)
def test_moments_bit_for_bit_on_exact_samples(widths, B, n_real, T, t_step, rows, pieces):
    inputs, traj = exact_samples(7, T, widths, B, n_real)
    want, _ = orc.moments(inputs, traj, rows, n_real, t_step)
    got, dropped = run_op(inputs, traj, rows, t_step, n_real, pieces)
    kept = len(range(0, T, t_step)) * n_real
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(got, got.T) and got[-1, -1] == kept and dropped == 0


@pytest.mark.parametrize("where", ["x", "y", "both"])
def test_dropped_samples(where):
    """Non-finite target values on scattered (t, b) — in the first target row only, in the second only, in both; NaN and
    both infinities — drop those samples entirely: nothing of them (their rates hold NaN as well) reaches a sum, and
    they are counted."""
    widths, B, n_real, T, t_step = (17, 33), 68, 66, 70, 2
    inputs, traj = exact_samples(9, T, widths, B, n_real)
    rng = np.random.RandomState(10)
    hit = rng.rand(T, B) < 0.07
    hit[0, 0] = hit[T - 2, n_real - 1] = True
    bad = rng.choice(np.float32([np.nan, np.inf, -np.inf]), size=(T, B))
    for r in {"x": (0,), "y": (1,), "both": (0, 1)}[where]:
        traj[:, r][hit] = bad[hit]
    for x in inputs:
        x.transpose(0, 2, 1)[hit] = np.nan
    traj[:, :, n_real:] = HUGE
    want, odropped = orc.moments(inputs, traj, (0, 1), n_real, t_step)
    assert odropped == int(hit[::t_step, :n_real].sum()) > 20
    got, dropped = run_op(inputs, traj, (0, 1), t_step, n_real, [(0, 36), (36, 70)])
    assert np.array_equal(got, want) and dropped == odropped
    assert got[-1, -1] == len(range(0, T, t_step)) * n_real - odropped


def test_real_rates_repeat_and_rounding_bound():
    rng = np.random.RandomState(4)
    widths, B, n_real, T, t_step = (33, 20), 200, 199, 70, 1
    inputs = [rng.rand(T, n, B).astype(np.float32) ** 3 for n in widths]
    traj = rng.randn(T, 8, B).astype(np.float32)
    a, _ = run_op(inputs, traj, (0, 1), t_step, n_real)
    b, _ = run_op(inputs, traj, (0, 1), t_step, n_real)
    assert np.array_equal(a, b)                                        # the same call, the same bits
    want, _ = orc.moments(inputs, traj, (0, 1), n_real, t_step)
    S = T * n_real
    bound = S * 2.0 ** -53 * orc.abs_moments(inputs, traj, (0, 1), n_real, t_step)
    err = np.abs(a - want)
    print(f"real rates: worst |error| / bound = {float((err / bound).max()):.3g} (S = {S})")
    assert (err <= bound).all() and np.array_equal(a, a.T)


GUARD_CASES = [c for c in EXACT_CASES if c[0] in ((1,), (17,), (17, 33), (33, 100, 17), (100,))][:6]


@pytest.mark.parametrize("widths, B, n_real, T, t_step, rows, pieces", GUARD_CASES)
def test_guard_bands(widths, B, n_real, T, t_step, rows, pieces):
    """moments, workspace and n_dropped inside canary-filled arenas: nothing outside the views is written, every double of
    the workspace is, and the results do not depend on what the memory held."""
    from ratinabox_amd import _lib as L
    inputs, traj = exact_samples(7, T, widths, B, n_real)
    want, _ = orc.moments(inputs, traj, rows, n_real, t_step)
    dx, dt = [torch.from_numpy(x).to(DEV) for x in inputs], torch.from_numpy(traj).to(DEV)
    m = want.shape[0]
    need = int(L.lib.riab_history_moments_workspace(T, t_step, m, B))
    assert need > 0 and need % 4096 == 0
    arr = (L.RiabMomentInput * len(dx))()
    for a, x in zip(arr, dx):
        a.rows, a.n = x.data_ptr(), int(x.shape[1])
    tr = (C.c_int32 * len(rows))(*rows)
    seen = None
    for canary in CANARIES:
        arena = GuardArena(canary)
        M = arena.view((m, m), torch.float64, DEV)
        ws = arena.view((need // 64, 64), torch.float64, DEV)   # (64 x 64 doubles per block pair and split)
        dropped = arena.view((1,), torch.int64, DEV)
        M.zero_()
        dropped.zero_()
        rc = L.lib.riab_history_moments(arr, len(dx), L.ptr(dt), tr, len(rows), T, t_step, B, n_real, L.ptr(M), L.ptr(dropped),
                                        L.ptr(ws), L.current_stream())
        assert rc == 0
        torch.cuda.synchronize()
        got = arena.check(M, other=None if seen is None else seen[0])
        w = arena.check(ws, other=None if seen is None else seen[1])
        assert int(arena.check(dropped)[0]) == 0 and np.array_equal(got, want)
        seen = (got, w)


def test_fixture_through_the_operators(G):
    """The reference's scenario as one agent (B = 4, n_real = 1), every 5th training row, alpha 0.01: float64 predictions
    from coef_ / intercept_ on the test rows against sklearn's.  Allowance 1e-7 m (an fp32 accumulation misses it by three
    to four orders of magnitude); measured on the MI355X: pc 1.3e-13 m, gc 6.7e-15 m, all 1.1e-13 m."""
    from ratinabox_amd._decoder import LinearDecoder, MomentLayout
    n_train, stride = int(G["n_train"]), int(G["stride"])
    T = len(G["pos"])
    traj = np.full((T, 8, 4), HUGE, dtype=np.float32)
    traj[:, 0, 0], traj[:, 1, 0] = G["pos"][:, 0], G["pos"][:, 1]
    for tag, cols in (("pc", slice(0, 20)), ("gc", slice(20, 40)), ("all", slice(0, 40))):
        rows = np.full((T, cols.stop - cols.start, 4), np.nan, dtype=np.float32)
        rows[:, :, 0] = G["fr"][:, cols]
        M = torch.zeros((rows.shape[1] + 3,) * 2, dtype=torch.float64, device=DEV)
        dropped = torch.zeros(1, dtype=torch.int64, device=DEV)
        torch.ops.riab.history_moments([torch.from_numpy(rows[:n_train]).to(DEV)], torch.from_numpy(traj[:n_train]).to(DEV),
                                       [0, 1], stride, 1, M, dropped)
        dec = LinearDecoder.from_moments(M, MomentLayout([rows.shape[1]], "pos", n_dropped=dropped), alpha=float(G["alpha"]))
        assert dec.coef_.device.type == "cuda" and dec.coef_.dtype == torch.float64
        assert dec.n_samples == len(range(0, n_train, stride)) and dec.n_dropped == 0
        pred = orc.predict(dec.coef_.cpu().numpy(), dec.intercept_.cpu().numpy(), G["fr"][n_train:, cols])
        err = float(np.abs(pred - G[f"pred_{tag}"]).max())
        print(f"{tag}: device fit against sklearn's predictions: {err:.3g} m")
        assert err <= 1e-7


@pytest.fixture(scope="module")
def live(riab):
    """10 agents (Bp = 12), 33 PlaceCells + 20 GridCells, 300 steps: simulate(37), 60 update() steps, simulate(150), 53
    update() steps.  The place cells' history was preallocated, so its chunk boundaries differ from the others'."""
    np.random.seed(5)
    env = riab.Environment({})
    ag = riab.Agent(env, {"n_agents": 10, "dt": 0.05, "seed": 21})
    pcs = riab.PlaceCells(ag, {"n": 33, "widths": 0.3})
    gcs = riab.GridCells(ag, {"n": 20})
    pcs._hist_fr.preallocate(400)

    def loop(k):
        for _ in range(k):
            ag.update()
            pcs.update()
            gcs.update()
    ag.simulate(37)
    loop(60)
    ag.simulate(150)
    loop(53)
    assert len(ag.history["t"]) == 300 and len(pcs.history["t"]) == 300    # (publishes the rows a step plan still holds)
    return dict(ag=ag, pcs=pcs, gcs=gcs)


def host_history(ag, pops):
    """(inputs [(T, n, Bp)], traj (T, 8, Bp)) float32 host copies of the device histories, padding lanes included."""
    return ([p.get_history_tensors()[0].cpu().numpy() for p in pops], ag.get_history_tensor().cpu().numpy())


def fp32_allowance(coef, icpt, x):
    """(n + 3) * 2^-24 * (sum_k |w_k r_k| + |b|) per decoded value; x (S, n) -> (S, D)"""
    n = coef.shape[1]
    return (n + 3) * 2.0 ** -24 * (np.abs(x).astype(np.float64) @ np.abs(coef).T + np.abs(icpt))


def test_through_the_classes(riab, live):
    ag, pcs, gcs = live["ag"], live["pcs"], live["gcs"]
    fa, fp, fg = ag._hist.filled, pcs._hist_fr.filled, gcs._hist_fr.filled
    assert sum(fa) == sum(fp) == sum(fg) == 300
    assert list(np.cumsum(fa)) != list(np.cumsum(fp)) and max(len(fa), len(fp), len(fg)) > 1, (fa, fp, fg)
    t = np.asarray(ag.history["t"])
    dec = riab.fit_linear_decoder([pcs, gcs], t_end=t[240], stride=2)
    assert dec.layout.rows == (0, 240, 2) and dec.n_samples == 120 * 10 and dec.n_dropped == 0
    assert tuple(dec.coef_.shape) == (2, 53) and dec.target == "pos" and dec.alpha == 0.01
    inputs, traj = host_history(ag, [pcs, gcs])
    M, _ = orc.moments([x[:240] for x in inputs], traj[:240], (0, 1), 10, 2)
    coef, icpt = orc.ridge(M, 53, 2, 0.01)
    x_all = np.concatenate(inputs, axis=1)[:, :, :10].transpose(0, 2, 1).reshape(-1, 53)        # (300 * 10, 53)
    got64 = orc.predict(dec.coef_.cpu().numpy(), dec.intercept_.cpu().numpy(), x_all)
    diff = float(np.abs(got64 - orc.predict(coef, icpt, x_all)).max())
    print(f"float64 predictions, device fit against the oracle's: {diff:.3g} m")
    assert diff <= 1e-8
    # the same decoder from one population through Neurons.fit_decoder
    one = pcs.fit_decoder(t_end=t[240], stride=2)
    M1, _ = orc.moments([inputs[0][:240]], traj[:240], (0, 1), 10, 2)
    c1, i1 = orc.ridge(M1, 33, 2, 0.01)
    x1 = x_all[:, :33]
    assert np.abs(orc.predict(one.coef_.cpu().numpy(), one.intercept_.cpu().numpy(), x1) - orc.predict(c1, i1, x1)).max() <= 1e-8
    # decode_tensor on the last 60 rows: fp32 matrix cores against the float64 decoder
    out = dec.decode_tensor(t_start=t[240])
    assert tuple(out.shape) == (60, 2, 12) and out.dtype == torch.float32 and out.device.type == "cuda"
    w, b = dec.coef_.cpu().numpy(), dec.intercept_.cpu().numpy()
    x_test = x_all.reshape(300, 10, 53)[240:]
    want = orc.predict(w, b, x_test.reshape(-1, 53)).reshape(60, 10, 2)
    allow = fp32_allowance(w, b, x_test.reshape(-1, 53)).reshape(60, 10, 2)
    got = out.cpu().numpy()[:, :, :10].transpose(0, 2, 1)
    print(f"decode_tensor: worst |error| / allowance = {float((np.abs(got - want) / allow).max()):.3g}")
    assert (np.abs(got - want) <= allow).all()
    dd = dec.decode(t_start=t[240])
    assert dd.shape == (60, 10, 2) and np.array_equal(dd, got)
    # error(): the mean distance to the recorded position, per agent
    pos = traj[240:, :2, :10].transpose(0, 2, 1).astype(np.float64)
    want_err = np.sqrt(((dd.astype(np.float64) - pos) ** 2).sum(axis=2)).mean(axis=0)
    e = dec.error(t_start=t[240])
    assert tuple(e.shape) == (10,) and e.device.type == "cuda"
    assert np.allclose(e.cpu().numpy(), want_err, rtol=1e-12, atol=0)
    print(f"decoding error on the held-out rows: {1000 * float(want_err.mean()):.1f} mm")


def test_decoder_as_a_live_layer(riab, live):
    ag, pcs, gcs = live["ag"], live["pcs"], live["gcs"]
    t = np.asarray(ag.history["t"])
    dec = riab.fit_linear_decoder([pcs, gcs], t_end=t[240], stride=2)
    w, b = dec.coef_.cpu().numpy(), dec.intercept_.cpu().numpy()
    layer = dec.as_layer()
    assert isinstance(layer, riab.FeedForwardLayer) and layer.n == 2 and list(layer.inputs) == [pcs.name, gcs.name]
    ag.update()
    pcs.update()
    gcs.update()
    layer.update()
    x = np.concatenate((pcs.firingrate, gcs.firingrate), axis=0).T                               # (10, 53)
    assert (np.abs(layer.firingrate.T - orc.predict(w, b, x)) <= fp32_allowance(w, b, x)).all()
    # ... and in a step plan, where its rows are recorded like any population's
    rows_before = len(layer._hist_fr)
    plan = ag.make_step_plan([pcs, gcs, layer])
    plan.step(3)
    plan.close()
    assert len(layer.history["t"]) == rows_before + 3
    fr = [p.get_history_tensors()[0].cpu().numpy()[-3:, :, :10] for p in (pcs, gcs)]
    x = np.concatenate(fr, axis=1).transpose(0, 2, 1).reshape(-1, 53)
    got = layer.get_history_tensors()[0].cpu().numpy()[-3:, :, :10].transpose(0, 2, 1).reshape(-1, 2)
    assert (np.abs(got - orc.predict(w, b, x)) <= fp32_allowance(w, b, x)).all()
