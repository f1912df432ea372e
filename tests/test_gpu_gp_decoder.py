"""The Gaussian-process decoder on the device (csrc/riab_gp.hip, ratinabox_amd/_gp_decoder.py) against the float64
restatement (tests/gp_decoder_oracle.py) and scikit-learn's own results on the reference's decoding scenario
(tests/golden/gp_decoder_reference.npz).

On one-hot problems (training vectors a squared distance >= 1 apart, 1 / (2 l^2) = 200: every off-sample term underflows to
0 in fp32 and every on-sample distance is exactly 0) the output is compared BIT FOR BIT with the alpha column of the sample.
On real rates the allowance per value is 8 * 2^-24 * sum_j |alpha_jd|: the fp32 emulation of the kernel's arithmetic stays
within 1 of that unit (tests/test_gp_decoder_cpu.py: 0.21-0.50 on the golden's tags, 0.21 at n = 1024, N = 4096, 0.50 at n = 20,
N = 8192), the
factor 8 is margin for v_exp_f32, FMA contraction and the summation order; a bf16 or fp16 cross term misses it by orders of
magnitude."""
import os

import numpy as np
import pytest
import torch

from tests import gp_decoder_oracle as orc
from tests.guard_arena import CANARIES, GuardArena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIO = os.path.join(ROOT, "tests", "golden", "decoder_reference.npz")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gp_decoder_reference.npz")
DEV = "cuda"
HUGE = np.float32(3.0e38)
UNIT = 2.0 ** -24
MARGIN = 8.0

# (widths, N, B, n_real, T, D): 1, 2 and 3 populations; every n of {1, 15, 16, 17, 33, 100} (K slabs of 16, ragged first rows);
# every N of {1, 31, 32, 33, 127, 129, 480} (32-row tiles; 32-, 64- and 128-sample blocks; 1, 2 and 4 blocks); every B of
# {4, 12, 64, 68, 200} with n_real 1-3 below it; T of {1, 3}; D of {1, 2, 4}
CASES = [
    ((1,), 1, 4, 3, 1, 1),
    ((15,), 31, 12, 10, 3, 2),
    ((16,), 32, 64, 63, 1, 4),
    ((17,), 33, 68, 65, 3, 2),
    ((33,), 127, 200, 197, 1, 1),
    ((100,), 129, 12, 9, 3, 2),
    ((1, 15), 480, 64, 62, 3, 4),
    ((17, 33), 31, 68, 67, 1, 2),
    ((16, 100), 129, 4, 2, 3, 1),
    ((15, 17, 33), 127, 200, 198, 3, 2),
    ((100, 1, 16), 33, 12, 11, 1, 4),
    ((33, 100, 17), 480, 68, 66, 3, 2),
]


@pytest.fixture(scope="module")
def riab():
    import ratinabox_amd
    return ratinabox_amd


def tables(X, alpha, widths):
    """what the operator takes: ([W^T (n_l, Np)], sq (Np,), alpha (D, Np)) float32 host arrays, zero padded"""
    N, Np = X.shape[0], (X.shape[0] + 31) // 32 * 32
    wts, k = [], 0
    for w in widths:
        wt = np.zeros((w, Np), dtype=np.float32)
        wt[:, :N] = X[:, k:k + w].T
        wts.append(wt)
        k += w
    sq = np.zeros(Np, dtype=np.float32)
    sq[:N] = (X.astype(np.float64) ** 2).sum(axis=1)
    al = np.zeros((alpha.shape[1], Np), dtype=np.float32)
    al[:, :N] = alpha.T
    return wts, sq, al


def split(Q, widths):
    """queries (T, B, n) -> the operator's inputs [(T, n_l, B)]"""
    out, k = [], 0
    for w in widths:
        out.append(np.ascontiguousarray(Q[:, :, k:k + w].transpose(0, 2, 1)))
        k += w
    return out


def run_op(inputs, X, alpha, widths, inv_two_ell2):
    import ratinabox_amd.ops  # noqa: F401  (registers torch.ops.riab.*)
    wts, sq, al = tables(X, alpha, widths)
    out = torch.ops.riab.gp_predict([torch.from_numpy(x).to(DEV) for x in inputs], [torch.from_numpy(w).to(DEV) for w in wts],
                                    torch.from_numpy(sq).to(DEV), torch.from_numpy(al).to(DEV), X.shape[0], float(inv_two_ell2))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def one_hot_problem(seed, widths, N, B, n_real, T, D):
    """Training vectors: the digits of j (base b, b^min(n, 3) >= N) in the first coordinates — integers, so two samples are a
    squared distance >= 1 apart — and multiples of 1 / 32 below 1 in the others: every product and partial sum is exact in
    fp32.  Query (t, b) is training sample `which[t, b]`, or, for which == N, a point 2 or more away from every sample."""
    rng = np.random.RandomState(seed)
    n = sum(widths)
    nd = min(n, 3)
    base = 1
    while base ** nd < N:
        base += 1
    X = (rng.randint(0, 32, size=(N, n)) / 32.0).astype(np.float32)
    j = np.arange(N)
    for c in range(nd):
        X[:, c] = (j // base ** c) % base
    assert len({tuple(x[:nd]) for x in X}) == N and (X.astype(np.float64) ** 2).sum(axis=1).max() * 1024 < 2 ** 23
    alpha = rng.randn(N, D).astype(np.float32)
    which = rng.randint(0, N + 1, size=(T, B))
    which[0, 0], which[-1, n_real - 1] = N - 1, 0
    if T * n_real > 2:
        which[0, 1 % n_real] = N
    Q = np.zeros((T, B, n), dtype=np.float32)
    on = which < N
    Q[on] = X[which[on]]
    far = (rng.randint(0, 32, size=(T, B, n)) / 32.0).astype(np.float32)
    far[:, :, 0] = -2.0 - rng.randint(0, 3, size=(T, B))
    Q[~on] = far[~on]
    Q[:, n_real:] = np.nan
    want = np.zeros((T, D, B), dtype=np.float32)
    for t in range(T):
        for b in range(n_real):
            if which[t, b] < N:
                want[t, :, b] = alpha[which[t, b]]
    return X, alpha, Q, want


@pytest.mark.parametrize("widths, N, B, n_real, T, D", CASES)
def test_one_hot_bit_for_bit(widths, N, B, n_real, T, D):
    X, alpha, Q, want = one_hot_problem(3, widths, N, B, n_real, T, D)
    got = run_op(split(Q, widths), X, alpha, widths, 200.0)
    assert got.shape == (T, D, B) and got.dtype == np.float32
    assert np.array_equal(got[:, :, :n_real].view(np.uint32), want[:, :, :n_real].view(np.uint32))
    assert (want[:, :, :n_real] != 0).any() and (want[:, :, :n_real] == 0).any()


def real_problem(seed, widths, N, B, n_real, T, D):
    rng = np.random.RandomState(seed)
    n = sum(widths)
    X = (rng.rand(N, n) ** 3).astype(np.float32)
    alpha = rng.randn(N, D).astype(np.float32)
    Q = (rng.rand(T, B, n) ** 3).astype(np.float32)
    Q[:, n_real:] = np.nan
    return X, alpha, Q, float(np.sqrt(n / 20.0))


WORST = {}


@pytest.mark.parametrize("widths, N, B, n_real, T, D", CASES)
def test_real_rates(widths, N, B, n_real, T, D):
    X, alpha, Q, ell = real_problem(5, widths, N, B, n_real, T, D)
    inv = 1.0 / (2.0 * ell * ell)
    inputs = split(Q, widths)
    got = run_op(inputs, X, alpha, widths, inv)
    want = orc.predict(Q[:, :n_real].reshape(T * n_real, -1), X, alpha.astype(np.float64), ell).reshape(T, n_real, D)
    err = np.abs(got[:, :, :n_real].transpose(0, 2, 1) - want)
    ratio = float((err / (UNIT * orc.l1(alpha))).max())
    WORST[(widths, N)] = ratio
    print(f"widths {widths}, N {N}, B {B}, T {T}, D {D}: worst |error| / (2^-24 |alpha|_1) = {ratio:.3g} "
          f"(worst so far {max(WORST.values()):.3g})")
    assert np.isfinite(got[:, :, :n_real]).all() and ratio <= MARGIN
    # the same call, the same bits; a row alone has the bits it has inside the many-row call
    again = run_op(inputs, X, alpha, widths, inv)
    assert np.array_equal(got[:, :, :n_real].view(np.uint32), again[:, :, :n_real].view(np.uint32))
    for t in range(T):
        alone = run_op([x[t:t + 1] for x in inputs], X, alpha, widths, inv)
        assert np.array_equal(alone[0, :, :n_real].view(np.uint32), got[t, :, :n_real].view(np.uint32))


@pytest.mark.parametrize("widths, N, B, n_real, T, D", [CASES[3], CASES[6], CASES[9]])
def test_poisoned_padding_and_one_poisoned_sample(widths, N, B, n_real, T, D):
    X, alpha, Q, ell = real_problem(6, widths, N, B, n_real, T, D)
    inv = 1.0 / (2.0 * ell * ell)
    clean = Q.copy()
    clean[:, n_real:] = 0.25
    base = run_op(split(clean, widths), X, alpha, widths, inv)
    for poison in (np.float32(np.nan), HUGE, np.float32(-np.inf)):
        Qp = Q.copy()
        Qp[:, n_real:] = poison
        got = run_op(split(Qp, widths), X, alpha, widths, inv)
        assert np.array_equal(got[:, :, :n_real].view(np.uint32), base[:, :, :n_real].view(np.uint32))
        # one real sample with one bad rate: its outputs are not finite, nobody else's change
        t, b, k = T - 1, n_real // 2, sum(widths) - 1
        Qp[t, b, k] = poison
        got = run_op(split(Qp, widths), X, alpha, widths, inv)
        assert not np.isfinite(got[t, :, b]).any()
        mask = np.ones((T, B), dtype=bool)
        mask[:, n_real:] = False
        mask[t, b] = False
        assert np.array_equal(got.transpose(0, 2, 1)[mask].view(np.uint32), base.transpose(0, 2, 1)[mask].view(np.uint32))


GUARD_CASES = [CASES[0], CASES[3], CASES[4], CASES[7], CASES[8], CASES[11]]


@pytest.mark.parametrize("widths, N, B, n_real, T, D", GUARD_CASES)
def test_guard_bands(widths, N, B, n_real, T, D):
    """`out` inside canary-filled arenas (there is no workspace: N is not split): nothing outside the view is written, every
    word of it is, and the results do not depend on what the memory held."""
    from ratinabox_amd import _lib as L
    X, alpha, Q, want = one_hot_problem(3, widths, N, B, n_real, T, D)
    wts, sq, al = tables(X, alpha, widths)
    dx = [torch.from_numpy(x).to(DEV) for x in split(Q, widths)]
    dw = [torch.from_numpy(w).to(DEV) for w in wts]
    dsq, dal = torch.from_numpy(sq).to(DEV), torch.from_numpy(al).to(DEV)
    arr = (L.RiabFFInput * len(dx))()
    for a, x, w in zip(arr, dx, dw):
        a.rates, a.wt, a.n_in = x.data_ptr(), w.data_ptr(), int(x.shape[1])
    seen = None
    for canary in CANARIES:
        arena = GuardArena(canary)
        out = arena.view((T, D, B), torch.float32, DEV)
        rc = L.lib.riab_gp_predict(arr, len(dx), L.ptr(dsq), L.ptr(dal), D, N, 200.0, T, B, L.ptr(out), L.current_stream())
        assert rc == 0
        torch.cuda.synchronize()
        got = arena.check(out, other=seen)
        assert np.array_equal(got[:, :, :n_real].view(np.uint32), want[:, :, :n_real].view(np.uint32))
        seen = got


# ---- the reference's scenario, replayed into the history of one agent ----------------------------------------------------
COLUMNS = {"pc": slice(0, 20), "gc": slice(20, 40), "all": slice(0, 40)}


def replayed_agent(riab, S):
    """One agent (Bp = 4, lane 0 real) whose trajectory and rate histories ARE the fixture's rows: 20 PlaceCells (columns
    0..19 of fr) and 20 GridCells (20..39); the padding lanes hold 3e38 positions and NaN rates."""
    np.random.seed(1)
    ag = riab.Agent(riab.Environment({}), {"dt": 0.05})
    pcs, gcs = riab.PlaceCells(ag, {"n": 20}), riab.GridCells(ag, {"n": 20})
    T = len(S["pos"])
    assert ag._B == 1 and ag._Bp == 4
    traj = np.full((T, 8, 4), HUGE, dtype=np.float32)
    traj[:, 0, 0], traj[:, 1, 0] = S["pos"][:, 0], S["pos"][:, 1]
    ag._hist.reserve(T).copy_(torch.from_numpy(traj))
    ag._times = [float(x) for x in S["t"]]
    for pop, cols in ((pcs, COLUMNS["pc"]), (gcs, COLUMNS["gc"])):
        rows = np.full((T, 20, 4), np.nan, dtype=np.float32)
        rows[:, :, 0] = S["fr"][:, cols]
        pop._hist_fr.reserve(T).copy_(torch.from_numpy(rows))
    return ag, pcs, gcs


def test_reference_scenario_through_the_class(riab):
    """Every 5th of the 2400 training rows, predictions on the 600 test rows: alpha_ against sklearn's with the CPU allowance
    64 cond 2^-53 max|alpha_|, decode_tensor against sklearn's predictions within 8 * 2^-24 * |alpha_d|_1 (7e-5 m for pc)."""
    S, G = dict(np.load(SCENARIO)), dict(np.load(GOLDEN))
    ag, pcs, gcs = replayed_agent(riab, S)
    n_train, stride = int(S["n_train"]), int(S["stride"])
    t = S["t"]
    for tag, pops in (("pc", [pcs]), ("gc", [gcs]), ("all", [pcs, gcs])):
        dec = riab.fit_gp_decoder(pops, t_end=t[n_train], stride=stride, alpha=float(G["alpha"]))
        assert isinstance(dec, riab.GPDecoder) and dec.alpha_.device.type == "cuda" and dec.alpha_.dtype == torch.float64
        assert dec.n_samples == 480 and dec.n_dropped == 0 and dec.length_scale == float(G[f"length_scale_{tag}"])
        assert np.array_equal(dec.train_rows.cpu().numpy(), np.arange(0, n_train, stride)) and not dec.train_agents.any()
        X = S["fr"][:n_train:stride, COLUMNS[tag]].astype(np.float64)
        assert np.array_equal(dec.X_train_.cpu().numpy(), X)
        want_a = G[f"alpha_{tag}"]
        cond = np.linalg.cond(orc.gram(X, dec.length_scale, dec.alpha))
        allow = 64.0 * cond * 2.0 ** -53 * np.abs(want_a).max()
        err_a = float(np.abs(dec.alpha_.cpu().numpy() - want_a).max())
        out = dec.decode_tensor(t_start=t[n_train])
        assert tuple(out.shape) == (600, 2, 4) and out.dtype == torch.float32
        got = out.cpu().numpy()[:, :, 0]
        bound = MARGIN * UNIT * orc.l1(want_a)
        err = np.abs(got - G[f"pred_{tag}"])
        print(f"{tag}: alpha_ against sklearn's {err_a:.3g} (allowance {allow:.3g}); decode_tensor against sklearn's predictions "
              f"{float(err.max()):.3g} m = {float((err / (UNIT * orc.l1(want_a))).max()):.3g} units (bound {bound.max():.3g} m)")
        assert err_a <= allow and (err <= bound).all()
        assert np.array_equal(dec.decode(t_start=t[n_train]), got)          # (one agent: (T, D))


# ---- a live batch ---------------------------------------------------------------------------------------------------------
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
    return ([p.get_history_tensors()[0].cpu().numpy() for p in pops], ag.get_history_tensor().cpu().numpy())


def check_fit(dec, X, y):
    """alpha_ against the oracle's fit on the same samples, allowance 64 cond 2^-53 max|alpha_|"""
    want = orc.fit(X, y, dec.length_scale, dec.alpha)
    cond = np.linalg.cond(orc.gram(X, dec.length_scale, dec.alpha))
    err, allow = float(np.abs(dec.alpha_.cpu().numpy() - want).max()), 64.0 * cond * 2.0 ** -53 * np.abs(want).max()
    print(f"alpha_ against the oracle's: {err:.3g} (allowance {allow:.3g}, cond {cond:.3g})")
    assert err <= allow
    return want


def test_through_the_classes(riab, live):
    ag, pcs, gcs = live["ag"], live["pcs"], live["gcs"]
    fa, fp = ag._hist.filled, pcs._hist_fr.filled
    assert sum(fa) == sum(fp) == 300 and list(np.cumsum(fa)) != list(np.cumsum(fp))
    t = np.asarray(ag.history["t"])
    dec = riab.fit_gp_decoder([pcs, gcs], t_end=t[240], stride=2, max_samples=512)
    ridx, agents = orc.select_samples(120, 10, 512)
    assert len(ridx) == 512 == dec.n_samples and dec.n_dropped == 0 and dec.target == "pos" and dec.alpha == 0.01
    assert np.array_equal(dec.train_rows.cpu().numpy(), 2 * ridx) and np.array_equal(dec.train_agents.cpu().numpy(), agents)
    assert dec.length_scale == np.sqrt(53 / 20) and tuple(dec.alpha_.shape) == (512, 2) and dec.alpha_.device.type == "cuda"
    inputs, traj = host_history(ag, [pcs, gcs])
    x_all = np.concatenate(inputs, axis=1).transpose(0, 2, 1).astype(np.float64)              # (300, 12, 53)
    X, y = x_all[2 * ridx, agents], traj[2 * ridx, :2, agents].astype(np.float64)
    assert np.array_equal(dec.X_train_.cpu().numpy(), X)
    check_fit(dec, X, y)
    # decode_tensor on the last 60 rows against the float64 mean of the decoder's own alpha_
    a64 = dec.alpha_.cpu().numpy()
    out = dec.decode_tensor(t_start=t[240])
    assert tuple(out.shape) == (60, 2, 12) and out.dtype == torch.float32 and out.device.type == "cuda"
    want = orc.predict(x_all[240:, :10].reshape(600, 53), X, a64, dec.length_scale).reshape(60, 10, 2)
    got = out.cpu().numpy()[:, :, :10].transpose(0, 2, 1)
    ratio = float((np.abs(got - want) / (UNIT * orc.l1(a64))).max())
    print(f"decode_tensor: worst |error| / (2^-24 |alpha_|_1) = {ratio:.3g}")
    assert ratio <= MARGIN
    assert torch.equal(dec.predict_tensor([torch.from_numpy(x[240:]).to(DEV) for x in inputs]), out)
    dd = dec.decode(t_start=t[240])
    assert dd.shape == (60, 10, 2) and np.array_equal(dd, got)
    pos = traj[240:, :2, :10].transpose(0, 2, 1).astype(np.float64)
    want_err = np.sqrt(((dd.astype(np.float64) - pos) ** 2).sum(axis=2)).mean(axis=0)
    e = dec.error(t_start=t[240])
    assert tuple(e.shape) == (10,) and e.device.type == "cuda" and np.allclose(e.cpu().numpy(), want_err, rtol=1e-12, atol=0)
    print(f"decoding error on the held-out rows: {1000 * float(want_err.mean()):.1f} mm")
    # one population through Neurons.fit_gp_decoder; everything fits under max_samples -> every candidate; samples= override
    one = gcs.fit_gp_decoder(t_end=t[40], stride=4, max_samples=100)
    r1, a1 = orc.select_samples(10, 10, 100)
    assert one.n_samples == 100 and np.array_equal(one.train_rows.cpu().numpy(), 4 * r1)
    assert np.array_equal(one.train_agents.cpu().numpy(), a1) and one.length_scale == 1.0
    check_fit(one, x_all[4 * r1, a1, 33:], traj[4 * r1, :2, a1].astype(np.float64))
    picked = pcs.fit_gp_decoder(t_end=t[240], stride=2, samples=([7, 3, 3, 119, 3, 7], [9, 0, 4, 2, 4, 9]), target="vel")   # (two pairs given twice)
    assert picked.n_samples == 4
    assert picked.train_rows.tolist() == [6, 6, 14, 238] and picked.train_agents.tolist() == [0, 4, 9, 2]
    check_fit(picked, x_all[[6, 6, 14, 238], [0, 4, 9, 2], :33], traj[[6, 6, 14, 238], 2:4, [0, 4, 9, 2]].astype(np.float64))


def test_samples_without_a_target_are_dropped(riab):
    """A ThetaSequenceAgent outside a sweep records NaN positions: such candidates are dropped and counted."""
    np.random.seed(8)
    ag = riab.Agent(riab.Environment({}), {"n_agents": 3, "dt": 0.05, "seed": 4})
    pcs = riab.PlaceCells(ag, {"n": 15})
    for _ in range(24):
        ag.update()
        pcs.update()
    assert len(ag.history["t"]) == 24
    hist = ag._hist.chunks[0]
    hist[4, 0, 1] = float("nan")          # row 4, agent 1: x
    hist[10, 1, 2] = float("inf")         # row 10, agent 2: y
    hist[5, 0, 0] = float("nan")          # row 5 is not selected at stride 2
    hist[6, 0, 3] = float("nan")          # a padding lane
    dec = pcs.fit_gp_decoder(stride=2)
    rows, agents = dec.train_rows.cpu().numpy(), dec.train_agents.cpu().numpy()
    assert dec.n_dropped == 2 and dec.n_samples == 12 * 3 - 2 == len(rows)
    pairs = set(zip(rows.tolist(), agents.tolist()))
    assert (4, 1) not in pairs and (10, 2) not in pairs and (4, 0) in pairs and (6, 2) in pairs
    assert torch.isfinite(dec.alpha_).all()
    e = dec.error()        # (rows with a NaN target are left out of the mean; agent 2's infinite one makes its mean infinite)
    assert tuple(e.shape) == (3,) and torch.isfinite(e[:2]).all()
    pcs._hist_fr.chunks[0][2, 3, 0] = float("nan")
    with pytest.raises(ValueError, match="rate is not finite"):
        pcs.fit_gp_decoder(stride=2)
