"""Rate maps and occupancy from the device history (csrc/riab_ratemap.hip) against the float64 restatement
(tests/ratemap_oracle.py = np.histogram2d on the widened fp32 samples) and the reference's own results
(tests/golden/ratemap_reference.npz).

Through the operators, on hand-made samples whose sums are exact in any order (rates k / 1024, fewer than 16384 samples
per bin), every output is compared BIT FOR BIT.  Through the classes, on real rates, the allowance per bin is derived:
|error| <= R * 2^-24 * sum|w| + S * 2^-52 * sum|w|, R = RIAB_RATEMAP_FP32_RUN (the longest fp32 run of the kernel; 0 = it
sums in float64 throughout), S = the largest number of samples in a bin (two float64 sums of at most S terms each, in
different orders, plus the rounding of the two divisions)."""
import os

import numpy as np
import pytest
import torch

from tests import ratemap_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ratemap_reference.npz")
DEV = "cuda"
HUGE = np.float32(3.0e38)


@pytest.fixture(scope="module")
def riab():
    import ratinabox_amd
    return ratinabox_amd


@pytest.fixture(scope="module")
def G():
    return dict(np.load(GOLDEN))


def run_ops(traj, rows, n_real, ex, ey, norm, pieces=None):
    """The three operators on host arrays traj (T, 8, B) float32, rows (T, n, B): (maps, zero_bins, counts, ids) as
    NumPy.  `pieces`: row ranges handed over one after the other, accumulating into the same buffers."""
    import ratinabox_amd.ops  # noqa: F401  (registers torch.ops.riab.*)
    nx, ny = len(ex) - 1, len(ey) - 1
    tx, ty = torch.from_numpy(np.ascontiguousarray(ex)), torch.from_numpy(np.ascontiguousarray(ey))
    counts = torch.zeros((ny, nx), dtype=torch.int64, device=DEV)
    sums = torch.zeros((rows.shape[1], ny, nx), dtype=torch.float64, device=DEV)
    dt, dr = torch.from_numpy(traj).to(DEV), torch.from_numpy(rows).to(DEV)
    all_ids = []
    for a, b in (pieces or [(0, traj.shape[0])]):
        ids = torch.ops.riab.history_bin_index(dt[a:b], tx, ty, n_real, counts)
        torch.ops.riab.history_rate_map(dr[a:b], ids, sums)
        all_ids.append(ids)
    maps, zero = torch.ops.riab.history_rate_map_finish(sums, counts, norm)
    torch.cuda.synchronize()
    return maps.cpu().numpy(), zero.cpu().numpy(), counts.cpu().numpy(), torch.cat(all_ids).cpu().numpy()


def make_traj(x, y, B):
    """Trajectory rows (T, 8, B) float32 from x, y (T, B); the other six rows hold a value that must never be read as a
    position."""
    T = x.shape[0]
    traj = np.full((T, 8, B), 0.5, dtype=np.float32)
    traj[:, 0], traj[:, 1] = x, y
    return traj


def exact_rates(rng, T, n, B, n_real):
    """k / 1024, k in [0, 1024): every partial sum of fewer than 16384 of them is exact in fp32 (and in float64) — and
    huge values in the padding lanes."""
    rows = (rng.randint(0, 1024, size=(T, n, B)) / 1024.0).astype(np.float32)
    rows[:, :, n_real:] = HUGE
    return rows



def check_against_oracle(traj, rows, n_real, ex, ey, pieces=None):
    for norm in (True, False):
        maps, zero, counts, _ = run_ops(traj, rows, n_real, ex, ey, norm, pieces)
        omaps, ozero, ocnt = orc.rate_maps(traj, rows, n_real, ex, ey, norm)
        assert ocnt.max() < 16384, "the premise of the bit-for-bit comparison: fewer than 16384 samples per bin"
        assert np.array_equal(counts, ocnt.astype(np.int64))
        assert zero.dtype == np.bool_ and np.array_equal(zero, ozero)
        assert maps.dtype == np.float64 and maps.shape == omaps.shape and np.array_equal(maps, omaps)


# ---- edges ---------------------------------------------------------------------------------------------------------
def special_values(e):
    """fp32 coordinates around every edge of e: the edge rounded to fp32, its fp32 neighbours, one ulp beyond the
    last edge, negative values, zeros of both signs, infinities and NaN."""
    f = e.astype(np.float32)
    v = np.concatenate((f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf)),
                        (0.5 * (e[1:] + e[:-1])).astype(np.float32),
                        np.array([-0.0, 0.0, -1.0, -1e-30, np.inf, -np.inf, np.nan, 1e30], dtype=np.float32)))
    return v.astype(np.float32)


@pytest.mark.parametrize("extent, dx", [((0, 1, 0, 1), 0.25), ((0, 2, 0, 1), 0.125), ((0, 1, 0, 1), 0.05),
                                         ((0, 2, 0, 1), 0.05), ((0, 0.3, 0, 0.2), 0.1), ((-0.5, 0.5, -0.25, 0.25), 0.05),
                                         ((0, 1, 0, 1), 1.5), ((0, 1, 0, 1), 0.04)])
def test_edges(extent, dx):
    """Positions on interior edges (dx 0.25 and 0.125: the edges are fp32 numbers), on the first and the last edge, one
    ulp beyond it, negative, NaN in x only or in y only; nx != ny; the (-0.5, 0.5) room with a position at exactly 0.5;
    a single-bin grid.  Counts and ids equal the searchsorted rule exactly."""
    ex, ey = orc.edges(extent, dx)
    xs, ys = special_values(ex), special_values(ey)
    if extent[0] == -0.5:
        xs = np.concatenate((xs, np.float32([0.5, -0.5])))
        ys = np.concatenate((ys, np.float32([0.25, -0.25])))
        assert orc.searchsorted_bins([0.5], ex)[0] == -1 and orc.searchsorted_bins([-0.5], ex)[0] == 0
    if dx == 1.5:
        assert len(ex) == 2 and len(ey) == 2
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    x, y = X.reshape(-1), Y.reshape(-1)
    P = len(x)
    B = (P + 3) // 4 * 4 + 4                      # (at least four padding lanes, holding a position inside the grid)
    inside = np.float32(0.5 * (ex[0] + ex[1])), np.float32(0.5 * (ey[0] + ey[1]))
    tx, ty = np.full((2, B), inside[0], dtype=np.float32), np.full((2, B), inside[1], dtype=np.float32)
    tx[0, :P], ty[0, :P] = x, y
    tx[1, :P], ty[1, :P] = x[::-1], y                # a second step with other pairs
    traj = make_traj(tx, ty, B)
    rows = exact_rates(np.random.RandomState(1), 2, 3, B, P)
    maps, zero, counts, ids = run_ops(traj, rows, P, ex, ey, True)
    nx, ny = len(ex) - 1, len(ey) - 1
    for t, (xx, yy) in enumerate(((x, y), (x[::-1], y))):
        kx, ky = orc.searchsorted_bins(xx, ex), orc.searchsorted_bins(yy, ey)
        want = np.where((kx >= 0) & (ky >= 0), (ny - 1 - ky) * nx + kx, -1)
        assert np.array_equal(ids[t, :P].astype(np.int64), want)
        assert (ids[t, P:] == -1).all()              # padding lanes never count
    assert np.array_equal(counts, orc.counts(traj, P, ex, ey).astype(np.int64)) and counts.shape == (ny, nx)
    omaps, ozero, _ = orc.rate_maps(traj, rows, P, ex, ey, True)
    assert np.array_equal(maps, omaps) and np.array_equal(zero, ozero)


# ---- shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3, 257])
@pytest.mark.parametrize("n", [1, 5, 33, 130])
@pytest.mark.parametrize("B, n_real", [(4, 4), (8, 5), (68, 68), (260, 260)])
def test_shapes_bit_for_bit(B, n_real, n, T):
    rng = np.random.RandomState(1000 * B + 10 * n + T)
    ex, ey = orc.edges((0, 2, 0, 1), 0.125)          # 16 x 8 bins; some samples fall outside
    x = rng.uniform(-0.1, 2.1, size=(T, B)).astype(np.float32)
    y = rng.uniform(-0.1, 1.1, size=(T, B)).astype(np.float32)
    x[:, n_real:], y[:, n_real:] = 1.0, 0.5            # padding lanes stand inside the room
    check_against_oracle(make_traj(x, y, B), exact_rates(rng, T, n, B, n_real), n_real, ex, ey)


# ---- collisions ----------------------------------------------------------------------------------------------------
def test_every_sample_in_one_bin():
    rng = np.random.RandomState(5)
    T, n, B = 3, 5, 260
    ex, ey = orc.edges((0, 1, 0, 1), 0.05)
    x = rng.uniform(0.51, 0.54, size=(T, B)).astype(np.float32)
    y = rng.uniform(0.26, 0.29, size=(T, B)).astype(np.float32)
    traj = make_traj(x, y, B)
    assert (orc.counts(traj, B, ex, ey) > 0).sum() == 1
    check_against_oracle(traj, exact_rates(rng, T, n, B, B), B, ex, ey)


def test_waves_alternate_between_two_bins():
    """Every agent of one wave instruction (64 lanes x 4 agents) in the same bin, neighbouring ones in another."""
    rng = np.random.RandomState(6)
    T, n, B = 2, 5, 1024
    ex, ey = orc.edges((0, 1, 0, 1), 0.05)
    which = (np.arange(B) // 256) % 2
    x = np.broadcast_to(np.where(which == 0, 0.12, 0.87).astype(np.float32), (T, B)).copy()
    y = np.broadcast_to(np.where(which == 0, 0.31, 0.68).astype(np.float32), (T, B)).copy()
    traj = make_traj(x, y, B)
    assert (orc.counts(traj, B, ex, ey) > 0).sum() == 2
    check_against_oracle(traj, exact_rates(rng, T, n, B, B), B, ex, ey)


# ---- spikes, accumulation, the bin cap -----------------------------------------------------------------------------
def test_spike_rows_are_exact():
    rng = np.random.RandomState(7)
    T, n, B, n_real = 5, 7, 72, 70
    ex, ey = orc.edges((0, 2, 0, 1), 0.125)
    x = rng.uniform(-0.1, 2.1, size=(T, B)).astype(np.float32)
    y = rng.uniform(-0.1, 1.1, size=(T, B)).astype(np.float32)
    rows = (rng.uniform(size=(T, n, B)) < 0.3).astype(np.uint8)
    rows[:, :, n_real:] = 255
    check_against_oracle(make_traj(x, y, B), rows, n_real, ex, ey)


def test_two_calls_accumulate_like_one():
    rng = np.random.RandomState(8)
    T, n, B, n_real = 6, 5, 68, 66
    ex, ey = orc.edges((0, 1, 0, 1), 0.25)
    x = rng.uniform(-0.1, 1.1, size=(T, B)).astype(np.float32)
    y = rng.uniform(-0.1, 1.1, size=(T, B)).astype(np.float32)
    traj, rows = make_traj(x, y, B), exact_rates(rng, T, n, B, n_real)
    one = run_ops(traj, rows, n_real, ex, ey, True)
    two = run_ops(traj, rows, n_real, ex, ey, True, pieces=[(0, 3), (3, 6)])
    for a, b in zip(one, two):
        assert np.array_equal(a, b)
    check_against_oracle(traj, rows, n_real, ex, ey, pieces=[(0, 1), (1, 6)])


def test_bin_cap():
    from ratinabox_amd import _lib
    rng = np.random.RandomState(9)
    T, n, B = 3, 5, 68
    assert _lib.RATEMAP_MAX_BINS >= 4096
    side = int(np.sqrt(_lib.RATEMAP_MAX_BINS))
    ex, ey = orc.edges((0, 1, 0, 1), 1.0 / side)
    assert (len(ex) - 1) * (len(ey) - 1) == _lib.RATEMAP_MAX_BINS     # just inside
    x = rng.uniform(-0.01, 1.01, size=(T, B)).astype(np.float32)
    y = rng.uniform(-0.01, 1.01, size=(T, B)).astype(np.float32)
    traj, rows = make_traj(x, y, B), exact_rates(rng, T, n, B, B)
    check_against_oracle(traj, rows, B, ex, ey)
    ex2 = np.arange(0.0, side + 2.0) / side                             # one more column: beyond
    assert (len(ex2) - 1) * (len(ey) - 1) > _lib.RATEMAP_MAX_BINS
    counts = torch.zeros((len(ey) - 1, len(ex2) - 1), dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.RiabError, match="not supported"):
        torch.ops.riab.history_bin_index(torch.from_numpy(traj).to(DEV), torch.from_numpy(ex2), torch.from_numpy(ey), B, counts)
    torch.cuda.synchronize()
    assert int(counts.sum()) == 0                                       # refused before launch


# ---- through the classes -------------------------------------------------------------------------------------------
def bound(sum_abs, counts, S, norm):
    from ratinabox_amd import _lib
    b = (_lib.RATEMAP_FP32_RUN * 2.0 ** -24 + S * 2.0 ** -52) * sum_abs
    return b / np.maximum(counts, 1) if norm else b


def load_history(riab, G, agent_chunks, pop_chunks, extra_row):
    """An agent and a 10-cell population whose device histories hold the fixture (one agent, padded to 4 lanes; the
    padding lanes hold positions inside the room and huge rates).  `extra_row`: one more recorded step behind the
    fixture's, so that the reference's slice (which leaves the last row out) selects exactly the fixture."""
    env = riab.Environment({"aspect": 2, "scale": 1})
    ag = riab.Agent(env, {"n_agents": 1, "dt": 0.05})
    N = riab.PlaceCells(ag, {"n": 10})
    pos, fr, sp, t = G["pos"], G["fr"], G["spikes"], list(G["t"])
    if extra_row:
        pos, fr, sp = np.concatenate((pos, pos[-1:])), np.concatenate((fr, fr[-1:])), np.concatenate((sp, sp[-1:]))
        t = t + [t[-1] + 0.05]
    T = len(pos)
    traj = np.full((T, 8, 4), 0.5, dtype=np.float32)
    traj[:, 0, 0], traj[:, 1, 0] = pos[:, 0], pos[:, 1]
    rates = np.full((T, 10, 4), HUGE, dtype=np.float32)
    rates[:, :, 0] = fr
    spikes = np.full((T, 10, 4), 255, dtype=np.uint8)
    spikes[:, :, 0] = sp

    def fill(hist, data, chunks):
        r = 0
        for k in list(chunks) + [T - sum(chunks)]:
            if k:
                hist.reserve(k).copy_(torch.from_numpy(data[r:r + k]))
                r += k
        assert len(hist) == T
    fill(ag._hist, traj, agent_chunks)
    fill(N._hist_fr, rates, pop_chunks)
    fill(N._hist_sp, spikes, pop_chunks)
    ag._times, N._times = list(t), list(t)
    return ag, N


@pytest.mark.parametrize("tag, dx", [("05", 0.05), ("10", 0.1)])
def test_fixture_replay(riab, G, tag, dx):
    ag, N = load_history(riab, G, agent_chunks=[700], pop_chunks=[300, 1200], extra_row=True)
    assert len(ag._hist.chunks) == 2 and len(N._hist_fr.chunks) == 3
    cnt = G[f"heatmap_{tag}"]
    S = cnt.max()
    sum_abs = G[f"rate_sum_{tag}"]                   # the rates are non-negative: sum|w| is the reference's own sum
    assert (G["fr"] >= 0).all()
    worst = 0.0
    for norm, ref in ((True, G[f"rate_norm_{tag}"]), (False, G[f"rate_sum_{tag}"])):
        maps, zero = N.get_rate_map(bin_size=dx, norm_by_bincount=norm)
        assert maps.dtype == np.float64 and maps.shape == ref.shape and np.array_equal(zero, G[f"zero_bins_{tag}"])
        err, b = np.abs(maps - ref), bound(sum_abs, cnt, S, norm)
        worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
        assert (err <= b).all()
    print(f"rate maps at dx {dx}: worst |error| / bound = {worst:.3g} (S = {int(S)})")
    # spike sums are integers: exact, and so are the quotients of two exactly known numbers
    for norm, ref in ((True, G[f"spike_norm_{tag}"]), (False, G[f"spike_sum_{tag}"])):
        maps, zero = N.get_rate_map(bin_size=dx, spikes=True, norm_by_bincount=norm)
        assert np.array_equal(maps, ref) and np.array_equal(zero, G[f"zero_bins_{tag}"])
    # the occupancy: the reference's call takes the whole history, last row included
    ag2, _ = load_history(riab, G, agent_chunks=[1999], pop_chunks=[], extra_row=False)
    h = ag2.get_position_heatmap(dx=dx)
    assert h.dtype == np.float64 and np.array_equal(h, cnt)
    assert torch.equal(ag2.get_position_heatmap_tensor(dx=dx).cpu(), torch.from_numpy(cnt.astype(np.int64)))


@pytest.fixture(scope="module")
def live(riab):
    """68 agents, 33 PlaceCells: simulate(37), simulate(50), then five update() steps."""
    np.random.seed(3)
    env = riab.Environment({})

    def run(seed, steps=(37, 50), updates=5):
        ag = riab.Agent(env, {"n_agents": 68, "dt": 0.05, "seed": seed})
        pcs = riab.PlaceCells(ag, {"n": 33})
        for s in steps:
            ag.simulate(s)
        for _ in range(updates):
            ag.update()
            pcs.update()
        return ag, pcs
    ag, pcs = run(11)
    return dict(ag=ag, pcs=pcs, other=run(12)[0], short=run(13, steps=(37,), updates=2)[0])


def host_rows(ag, N, spikes=False):
    """(traj (T, 8, B) float32, rows (T, n, B)) rebuilt from history[...] on the host."""
    pos = np.asarray(ag.history["pos"])
    traj = np.zeros((pos.shape[0], 8, pos.shape[1]), dtype=np.float32)
    traj[:, 0], traj[:, 1] = pos[..., 0], pos[..., 1]
    rows = np.asarray(N.history["spikes" if spikes else "firingrate"])
    return traj, np.ascontiguousarray(rows.astype(np.uint8) if spikes else rows)


def assert_within_bound(maps, zero, traj, rows, ex, ey, norm, label):
    omaps, ozero, ocnt = orc.rate_maps(traj, rows, traj.shape[2], ex, ey, norm)
    sum_abs = orc.rate_maps(traj, np.abs(rows), traj.shape[2], ex, ey, False)[0]
    b = bound(sum_abs, ocnt, ocnt.max(), norm)
    err = np.abs(maps - omaps)
    assert np.array_equal(zero, ozero) and maps.shape == omaps.shape and (err <= b).all()
    if (b > 0).any():
        print(f"{label}: worst |error| / bound = {float((err[b > 0] / b[b > 0]).max()):.3g}")


def test_live_run(live):
    ag, pcs = live["ag"], live["pcs"]
    T = 37 + 50 + 5
    assert len(ag.history["t"]) == T and len(pcs.history["t"]) == T   # (publishes the rows a step plan still holds)
    assert len(ag._hist) == T and len(pcs._hist_fr) == T
    assert len(ag._hist.chunks) > 1 or len(pcs._hist_fr.chunks) > 1, "the run must span several chunks"
    ex, ey = orc.edges((0, 1, 0, 1), 0.05)
    traj, rows = host_rows(ag, pcs)
    for norm in (True, False):
        maps, zero = pcs.get_rate_map(norm_by_bincount=norm)
        assert maps.shape == (33, 20, 20) and zero.shape == (20, 20)
        # the same rows through the operators, on the stacked tensors (the summation order differs where the chunks
        # end, so: the same numbers up to the order of float64 additions)
        full, (fr, _sp) = ag.get_history_tensor(), pcs.get_history_tensors()
        counts = torch.zeros((20, 20), dtype=torch.int64, device=DEV)
        sums = torch.zeros((33, 20, 20), dtype=torch.float64, device=DEV)
        ids = torch.ops.riab.history_bin_index(full[:T - 1].contiguous(), torch.from_numpy(ex), torch.from_numpy(ey), 68, counts)
        torch.ops.riab.history_rate_map(fr[:T - 1].contiguous(), ids, sums)
        omaps, ozero = torch.ops.riab.history_rate_map_finish(sums, counts, norm)
        assert np.array_equal(zero, ozero.cpu().numpy())
        assert_within_bound(omaps.cpu().numpy(), ozero.cpu().numpy(), traj[:T - 1], rows[:T - 1], ex, ey, norm, "operators")
        assert_within_bound(maps, zero, traj[:T - 1], rows[:T - 1], ex, ey, norm, "classes (last row left out)")
    # spikes
    straj, srows = host_rows(ag, pcs, spikes=True)
    maps, zero = pcs.get_rate_map(spikes=True, norm_by_bincount=False)
    assert np.array_equal(maps, orc.rate_maps(straj[:T - 1], srows[:T - 1], 68, ex, ey, False)[0])
    # t_start / t_end select the reference's rows, endid excluded
    t = np.asarray(ag.history["t"])
    maps, zero = pcs.get_rate_map(t_start=t[10], t_end=t[60])
    sl = ag.get_history_slice(t[10], t[60])
    assert (sl.start, sl.stop) == (10, 60)
    assert_within_bound(maps, zero, traj[10:60], rows[10:60], ex, ey, True, "rows [10, 60)")
    with pytest.raises(AssertionError):   # (row 60 is not part of it: the selection is told apart from [10, 61))
        assert_within_bound(maps, zero, traj[10:61], rows[10:61], ex, ey, True, "rows [10, 61)")
    # an empty selection
    maps, zero = pcs.get_rate_map(t_start=t[5], t_end=t[5])
    assert maps.shape == (33, 20, 20) and not maps.any() and zero.all()
    # the occupancy of the whole run, last row included; and of a selection
    assert np.array_equal(ag.get_position_heatmap(), orc.counts(traj, 68, ex, ey))
    assert np.array_equal(ag.get_position_heatmap(t_start=t[10], t_end=t[60]), orc.counts(traj[10:60], 68, ex, ey))
    # the ground truth on the environment's grid, for comparison
    gt, gz = pcs.get_rate_map(method="groundtruth")
    assert gt.shape == (33,) + ag.Environment.discrete_coords.shape[:2] and not gz.any()
    assert np.array_equal(gt.reshape(33, -1), pcs.get_state(evaluate_at="all"))


def test_same_call_twice_gives_the_same_bits(live):
    a = live["pcs"].get_rate_map_tensor()
    b = live["pcs"].get_rate_map_tensor()
    assert a[0].dtype == torch.float64 and a[1].dtype == torch.bool and a[0].is_cuda
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_position_data_agent(live):
    ag, pcs, other = live["ag"], live["pcs"], live["other"]
    ex, ey = orc.edges((0, 1, 0, 1), 0.05)
    _, rows = host_rows(ag, pcs)
    traj, _ = host_rows(other, pcs)
    assert not np.array_equal(traj, host_rows(ag, pcs)[0])
    maps, zero = pcs.get_rate_map(position_data_agent=other)
    assert_within_bound(maps, zero, traj[:-1], rows[:-1], ex, ey, True, "another agent's positions")


def test_length_mismatch_raises(live):
    with pytest.raises(ValueError, match="one position per recorded row"):
        live["pcs"].get_rate_map(position_data_agent=live["short"])
