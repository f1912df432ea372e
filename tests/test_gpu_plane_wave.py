"""contribs.PlaneWaveNeurons on the device (csrc/riab_rate_cells.h: PlaneWaveCell) against the reference's record
(tests/golden/plane_wave_*.npz) and the float64 oracle tests/plane_wave_oracle.py, which tests/test_plane_wave_cpu.py pins
to the reference.

Tolerance of a rate, per cell (plane_wave_oracle.tolerance): (max_fr - min_fr) (pi 2 (4 M_i + 3) 2^-24 + E_COS).  The phase is
fp32 revolutions; its error is bounded by (4 M_i + 3) 2^-24 with M_i = max_p (|x bx_i| + |y by_i|) over the positions of
the comparison (the rounding of a, of b, of the fp32 position and two arithmetic roundings); the rate's slope
in the phase is at most pi; 2 is margin.  E_COS is the absolute allowance the GridCells parity test
(tests/test_gpu_parity.py::test_grid_cells_vs_reference: floor 1.0 x RTOL x range) grants the same v_cos_f32 path.  At
lambda = 0.02 in the 2 x 1 m room that is about 2e-4 of the range; a wrong sign, offset or scale is an error of order 1.

Shapes are the smallest at which the kernels can still go wrong: n in {1, 3, 4, 5} around the wide kernel's group of 4 cells,
{8, 9, 17} around the row-following kernel's 8; B = 1 and 3 (padding to 4), 256 (the streamed lead population), 260 (no
multiple of 256: the trajectory path), 1024 positions (the wide kernel; fewer take the generic one); 20 steps and 300 (more
than 256: the row-following kernel's LONG variant)."""
import os

import numpy as np
import pytest
import torch

from oracle import riab_oracle as orc
from tests import golden_util as gu
from tests import plane_wave_oracle as pwo
from tests.test_gpu_parity import RTOL

pytestmark = pytest.mark.gpu

E_COS = 1.0 * RTOL      # (assert_rates(..., floor=1.0) in test_grid_cells_vs_reference: floor * RTOL * range)
FILES = sorted(f for f in os.listdir(gu.GOLDEN) if f.startswith("plane_wave_") and f.endswith(".npz"))


@pytest.fixture(scope="module")
def riab():
    assert torch.cuda.is_available(), "these tests need the GPU"
    import ratinabox_amd
    return ratinabox_amd


def _PW():
    from ratinabox_amd.contribs.PlaneWaveNeurons import PlaneWaveNeurons
    return PlaneWaveNeurons


def _golden_population(riab, g, cells=None, n_agents=1):
    """The population of a golden file (or of the rows `cells` of its arrays) on a fresh agent."""
    env = riab.Environment({"boundary_conditions": "periodic" if bool(g["periodic"]) else "solid", "aspect": float(g["aspect"]),
                            "scale": float(g["scale"])})
    ag = riab.Agent(env, {"n_agents": n_agents})
    cells = np.arange(int(g["n"])) if cells is None else np.asarray(cells)
    N = _PW()(ag, {"n": len(cells), "wavescale": float(g["wavescale"]), "min_fr": float(g["min_fr"]), "max_fr": float(g["max_fr"])})
    N.phase_offsets, N.w, N.wavescales = g["phase_offsets"][cells].copy(), g["w"][cells].copy(), g["wavescales"][cells].copy()
    return env, ag, N


def _check(got, ref, tab, pos, fr_range, what):
    """Every cell, every position: |got - ref| within the cell's allowance; the worst ratio is printed first."""
    tol = pwo.tolerance(tab, pos, fr_range, E_COS)[:, None]
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    c, p = np.unravel_index(np.argmax(err / tol), err.shape)
    print(f"[{what}] worst |err| / allowance = {(err / tol).max():.3f} (cell {c}, position {p}: |err| {err[c, p]:.2e}, "
          f"allowance {tol[c, 0]:.2e}); worst |err| / range = {err.max() / fr_range:.2e}")
    assert got.shape == ref.shape and (err <= tol).all()


# ---- 1. the kernels against the reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["generic", "wide"])
@pytest.mark.parametrize("name", FILES)
def test_kernel_vs_reference(riab, name, kernel):
    """get_state(evaluate_at=None, pos=...) — the registered operator — on the golden positions: 256 take the generic
    kernel, the same positions four times over (1024) the wide one."""
    g = gu.load(name)
    env, ag, N = _golden_population(riab, g)
    reps = 4 if kernel == "wide" else 1
    pos = np.tile(g["pos"], (reps, 1))
    got = N.get_state(evaluate_at=None, pos=pos)
    fr_range = float(g["max_fr"]) - float(g["min_fr"])
    tab = N._call(None, None)["table"].cpu().numpy()
    _check(got, np.tile(g["fr"], (1, reps)), tab, g["pos"], fr_range, f"{name} {kernel}")
    assert got.min() >= float(g["min_fr"]) and got.max() <= float(g["max_fr"])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 8, 9, 17])
def test_cell_group_edges_vs_reference(riab, n):
    """n cells around the group sizes of both kernels (4 and 8), drawn from the hand-assigned golden (lambda 0.02 .. 5, axis-aligned
    and diagonal w): positions 1024 (wide), 256 and 3 (generic, padded to 4)."""
    g = gu.load("plane_wave_assigned.npz")
    cells = np.arange(n) % int(g["n"])
    env, ag, N = _golden_population(riab, g, cells)
    tab = N._call(None, None)["table"].cpu().numpy()
    for P in (1024, 256, 3):
        pos = np.tile(g["pos"], (4, 1))[:P]
        got = N.get_state(evaluate_at=None, pos=pos)
        _check(got, np.tile(g["fr"][cells], (1, 4))[:, :P], tab, pos, 1.0, f"n={n} P={P}")


def test_evaluate_at_all_and_agent(riab):
    g = gu.load("plane_wave_assigned.npz")
    for B in (1, 3):                                       # (padding to 4 lanes)
        env, ag, N = _golden_population(riab, g, n_agents=B)
        coords = env.flattened_discrete_coords
        all_ = N.get_state(evaluate_at="all")
        assert all_.shape == (12, len(coords)) and np.array_equal(all_, N.get_state(evaluate_at=None, pos=coords))
        tab = N._call(None, None)["table"].cpu().numpy()
        _check(all_, pwo.rates(coords, g["phase_offsets"], g["w"], g["wavescales"]), tab, coords, 1.0, f"all B={B}")
        at = N.get_state()                                 # evaluate_at="agent"
        pos = np.asarray(ag.pos, dtype=np.float64).reshape(-1, 2)
        assert at.shape == (12, B)
        _check(at, pwo.rates(pos, g["phase_offsets"], g["w"], g["wavescales"]), tab, pos, 1.0, f"agent B={B}")
        ag.update()
        N.update()
        fr = np.asarray(N.firingrate, dtype=np.float64).reshape(12, B)
        row = ag.get_history_tensor()[-1].cpu().numpy().astype(np.float64)
        pos = np.stack((row[0], row[1]), -1)[:B]
        _check(fr, pwo.rates(pos, g["phase_offsets"], g["w"], g["wavescales"]), tab, pos, 1.0, f"update B={B}")


# ---- 2. every way of stepping gives the same bits ----------------------------------------------------------------------
DT, SEED = 0.01, 5


def _world(riab, B, n, spikes, with_place=False):
    np.random.seed(11)
    env = riab.Environment({})
    ag = riab.Agent(env, {"n_agents": B, "dt": DT, "seed": SEED})
    pcs = riab.PlaceCells(ag, {"n": 1024, "wall_geometry": "euclidean", "save_spikes": spikes}) if with_place else None
    N = _PW()(ag, {"n": n, "wavescale": 0.1, "min_fr": 0.5, "max_fr": 12.0, "save_spikes": spikes})
    return env, ag, pcs, N


def _collect(ag, pcs, N):
    torch.cuda.synchronize()
    fr, sp = N.get_history_tensors()
    out = {"traj": ag.get_history_tensor().cpu().numpy(), "state": ag.state_tensor.cpu().numpy(), "fr": fr.cpu().numpy(),
           "sp": sp.cpu().numpy(), "t": np.array(N.history["t"])}
    if pcs is not None:
        out["pc_fr"] = pcs.get_history_tensors()[0].cpu().numpy()
    return out


def _run(riab, mode, T, B, n, spikes, with_place=False):
    """One run of T steps from the same seed and start; returns its rows and the form of the rate stage (simulate)."""
    old = os.environ.get("RIAB_NO_AUTO_PLAN")
    if mode == "eager":
        os.environ["RIAB_NO_AUTO_PLAN"] = "1"
    try:
        env, ag, pcs, N = _world(riab, B, n, spikes, with_place)
        pops = [p for p in (pcs, N) if p is not None]
        form = None
        if mode in ("eager", "auto"):
            for _ in range(T):
                ag.update()
                for p in pops:
                    p.update()
        elif mode == "plan":
            plan = ag.make_step_plan()
            plan.step(1)
            for _ in range(min(T - 1, 4)):
                plan.step(1)
            if T > 5:
                plan.step(T - 5)
            plan.close()
        else:
            if mode == "strict":
                ag.pipeline_mode(strict=True)
            ag.simulate(T)
            form = ag.last_rate_stage_form()
            assert ag.engine_runs["native"] == 1 and ag.engine_runs["plan"] == 0 and ag.engine_runs["chunks"] == 0
    finally:
        if mode == "eager":
            os.environ.pop("RIAB_NO_AUTO_PLAN") if old is None else os.environ.__setitem__("RIAB_NO_AUTO_PLAN", old)
    return _collect(ag, pcs, N), form, N


def _same(got, ref, rows, what):
    for k in ref:
        a = got[k]
        b = ref[k] if k == "state" else ref[k][:rows]
        if k == "state" and rows != len(ref["fr"]):
            continue                                       # (a shorter run ends in another state)
        assert a.shape == b.shape and np.array_equal(a, b), (what, k)


def _rows_are_the_operator(riab, res, N):
    """Each rate row is the registered operator applied to the run's own history positions, bit for bit."""
    from ratinabox_amd import ops  # noqa: F401
    tab = N._call(None, None)["table"]
    traj = torch.from_numpy(res["traj"]).cuda()
    for t in range(traj.shape[0]):
        want = torch.ops.riab.plane_wave_neurons(traj[t, 0:2].contiguous(), tab, float(N.min_fr), float(N.max_fr))
        assert np.array_equal(want.cpu().numpy(), res["fr"][t]), t


@pytest.mark.parametrize("spikes", [False, True])
def test_every_way_of_stepping_gives_the_same_bits(riab, spikes):
    B, n, T = 256, 17, 300
    ref, _, N = _run(riab, "eager", T, B, n, spikes)
    assert ref["fr"].shape == (T, n, B) and np.isfinite(ref["fr"]).all() and ref["fr"].min() >= 0.5 and ref["fr"].max() <= 12.0
    if spikes:
        assert ref["sp"].shape == ref["fr"].shape and 0 < ref["sp"].mean() < 0.5
    _rows_are_the_operator(riab, ref, N)
    for mode, steps in (("auto", T), ("plan", T), ("simulate", 20), ("simulate", T), ("strict", 20), ("strict", T)):
        got, form, _ = _run(riab, mode, steps, B, n, spikes)
        _same(got, ref, steps, f"{mode} {steps}")
        if form is not None:                               # the population leads the row-following kernel: one kernel, all rows
            assert form == "one-kernel", (mode, steps, form)


@pytest.mark.parametrize("spikes", [False, True])
def test_not_the_lead_and_the_trajectory_path_give_the_same_bits(riab, spikes):
    # PlaceCells (1024) + PlaneWaveNeurons (9): the larger population leads, or neither does; PlaneWaveNeurons runs its
    # ordinary kernel either way
    T = 20
    ref, _, N = _run(riab, "eager", T, 256, 9, spikes, with_place=True)
    _rows_are_the_operator(riab, ref, N)
    for mode in ("plan", "simulate", "strict"):
        got, form, _ = _run(riab, mode, T, 256, 9, spikes, with_place=True)
        _same(got, ref, T, f"with PlaceCells, {mode}")
        assert form in (None, "populations", "chunks")
    # B = 260 is no multiple of 256: stream_supported refuses, the chunk form serves the run
    ref, _, N = _run(riab, "eager", T, 260, 8, spikes)
    _rows_are_the_operator(riab, ref, N)
    for mode in ("plan", "simulate", "strict"):
        got, form, _ = _run(riab, mode, T, 260, 8, spikes)
        _same(got, ref, T, f"B=260, {mode}")
        assert form in (None, "chunks")


# ---- 3. closed loop against the oracle ---------------------------------------------------------------------------------
def test_closed_loop_against_the_oracle(riab):
    """256 agents x 17 cells x 300 steps of update(): every rate against the oracle at the recorded fp32 history positions."""
    np.random.seed(3)
    B, n, T = 256, 17, 300
    ag = riab.Agent(riab.Environment({}), {"n_agents": B, "dt": DT, "seed": 9})
    N = _PW()(ag, {"n": n, "wavescale": 0.1, "min_fr": 0.5, "max_fr": 12.0, "save_spikes": False})
    for _ in range(T):
        ag.update()
        N.update()
    torch.cuda.synchronize()
    traj = ag.get_history_tensor().cpu().numpy().astype(np.float64)
    fr = N.get_history_tensors()[0].cpu().numpy()
    assert fr.shape == (T, n, B)
    pos = np.stack((traj[:, 0, :B], traj[:, 1, :B]), -1).reshape(-1, 2)           # (T * B, 2), step-major
    ref = pwo.rates(pos, N.phase_offsets, N.w, N.wavescales, 0.5, 12.0).reshape(n, T, B).transpose(1, 0, 2)
    tab = N._call(None, None)["table"].cpu().numpy()
    got = fr.transpose(1, 0, 2).reshape(n, T * B)
    _check(got, ref.transpose(1, 0, 2).reshape(n, T * B), tab, pos, 11.5, "closed loop")
    assert np.array_equal(np.asarray(N.history["firingrate"])[-1], fr[-1].astype(np.float64))


# ---- 4. the affine map and NaN positions -------------------------------------------------------------------------------
def test_affine_map_and_nan_positions(riab):
    g = gu.load("plane_wave_assigned.npz")
    for P in (256, 1024):                                  # the generic and the wide kernel
        pos = np.tile(g["pos"], (4, 1))[:P]
        _, _, unit = _golden_population(riab, g)
        _, _, wide = _golden_population(riab, g)
        wide.min_fr, wide.max_fr = 0.5, 10.0
        r01, r = unit.get_state(evaluate_at=None, pos=pos), wide.get_state(evaluate_at=None, pos=pos)
        assert r.min() >= 0.5 and r.max() <= 10.0 and r01.min() >= 0.0 and r01.max() <= 1.0
        # the [0, 1] rate is the same fp32 value in both populations (x 1 + 0 is exact); the map 0.5 + 9.5 r is a product and
        # a sum below 16, fused or not: at most two roundings of half an ulp of [8, 16), 2^-21 each
        np.testing.assert_allclose(r, 0.5 + 9.5 * r01, rtol=0, atol=2 * 2.0 ** -21)
        bad = pos.copy()
        bad[5] = np.nan
        bad[P - 1, 0] = np.nan
        got = wide.get_state(evaluate_at=None, pos=bad)
        assert (got[:, 5] == 0).all() and (got[:, P - 1] == 0).all() and np.isfinite(got).all()
        keep = np.ones(P, dtype=bool)
        keep[[5, P - 1]] = False
        assert np.array_equal(got[:, keep], r[:, keep])


# ---- 5. plans ---------------------------------------------------------------------------------------------------------
def test_plan_keeps_fusing_place_cells_and_takes_one_more_launch(riab):
    def run(with_pw):
        np.random.seed(4)
        ag = riab.Agent(riab.Environment({}), {"n_agents": 1024, "dt": 0.01, "seed": 2})
        pcs = riab.PlaceCells(ag, {"n": 40, "wall_geometry": "euclidean"})
        N = _PW()(ag, {"n": 9}) if with_pw else None
        plan = ag.make_step_plan()
        plan.step(1)
        torch.cuda.synchronize()
        base = plan.info()
        plan.step(20)
        info = plan.info()
        plan.close()
        torch.cuda.synchronize()
        return base, info, [pcs.get_history_tensors()[0].cpu().numpy(), ag.get_history_tensor().cpu().numpy()], N

    b0, i0, out0, _ = run(False)
    b1, i1, out1, N = run(True)
    assert i0["fused_populations"] == [0] == i1["fused_populations"]
    assert i0["fused_steps"] == 21 == i1["fused_steps"]
    per_step0 = (i0["launches"] - b0["launches"]) / 20
    per_step1 = (i1["launches"] - b1["launches"]) / 20
    print(f"[launches per step] PlaceCells: {per_step0:g}; + PlaneWaveNeurons: {per_step1:g}")
    assert per_step0 == 1 and per_step1 == 2
    for a, b in zip(out0, out1):
        assert np.array_equal(a, b)
    assert N.get_history_tensors()[0].shape == (21, 9, 1024)


# ---- 6. spikes and OU noise -------------------------------------------------------------------------------------------
def test_spikes_follow_the_rule_on_regenerated_uniforms(riab):
    np.random.seed(6)
    T, dt, seed = 6, 0.01, 77
    for B in (1024, 64):                                   # the wide and the generic kernel
        ag = riab.Agent(riab.Environment({}), {"n_agents": B, "dt": dt, "seed": seed})
        N = _PW()(ag, {"n": 9, "max_fr": 40.0, "min_fr": 1.0})
        for _ in range(T):
            ag.update()
            N.update()
        fr, sp = N.get_history_tensors()
        fr, sp = fr.cpu().numpy(), sp.cpu().numpy().astype(bool)
        for t in range(T):
            u = orc.spike_uniforms(seed, t + 1, N.pop_id, N.n, B)
            assert np.array_equal(sp[t], orc.spikes_f32(fr[t], u, dt)), (B, t)
        assert 0 < sp.mean() < 0.5
    u = np.random.uniform(size=(9, 64)).astype(np.float32)  # explicit uniforms
    ag.update()
    N.update(spike_uniforms=u)
    fr, sp = N.get_history_tensors()
    assert np.array_equal(sp[-1].cpu().numpy().astype(bool), orc.spikes_f32(fr[-1].cpu().numpy(), u, dt))


def test_ou_noise_is_added_as_for_any_population(riab):
    B, dt, seed = 256, 0.01, 21

    def mk(std):
        np.random.seed(8)          # (the same start and the same cells for both agents)
        ag = riab.Agent(riab.Environment({}), {"n_agents": B, "dt": dt, "seed": seed})
        return _PW()(ag, {"n": 8, "noise_std": std, "noise_coherence_time": 0.3, "max_fr": 5.0})

    clean, noisy = mk(0.0), mk(0.2)
    assert np.array_equal(clean.wavescales, noisy.wavescales)
    x = noisy._noise.clone()
    for step in range(1, 4):
        for pop in (clean, noisy):
            pop.Agent.update()
            pop.update()
        z = orc.noise_normals(seed, step, noisy.pop_id, 8, B)
        theta_dt, sigma_dt = noisy._noise_constants(dt)
        x = x + (-np.float32(theta_dt)) * x + np.float32(sigma_dt) * torch.from_numpy(z.astype(np.float32)).cuda()
        diff = (noisy.firingrate_tensor - clean.firingrate_tensor).cpu().numpy()
        # riab_neuron_noise: the fp32 rounding of rate + noise (rates below 8: half an ulp is 2.4e-7) and the hardware
        # log / cos of the draw (1e-6 of z, times sigma_dt = 0.05): the allowance of the theta tests
        np.testing.assert_allclose(diff, x.cpu().numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(noisy.noise, x.cpu().numpy().astype(np.float64), rtol=0, atol=1e-6)
    # a noisy population in simulate(): not streamed, same rows as the loop
    a, b = mk(0.2), mk(0.2)
    for _ in range(12):
        a.Agent.update()
        a.update()
    b.Agent.simulate(12)
    torch.cuda.synchronize()
    assert b.Agent.last_rate_stage_form() == "chunks"
    assert torch.equal(a.get_history_tensors()[0], b.get_history_tensors()[0])


# ---- 7. consumers -----------------------------------------------------------------------------------------------------
def test_feedforward_successor_features_and_rate_maps(riab):
    from ratinabox_amd.contribs.SuccessorFeatures import SuccessorFeatures
    np.random.seed(12)
    B, T = 64, 300
    env = riab.Environment({})
    ag = riab.Agent(env, {"n_agents": B, "dt": 0.01, "seed": 31})
    N = _PW()(ag, {"n": 17, "wavescale": 0.3, "save_spikes": False})
    feats = riab.PlaceCells(ag, {"n": 4, "wall_geometry": "euclidean", "save_spikes": False})
    ff = riab.FeedForwardLayer(ag, {"n": 5, "input_layers": [N], "name": "F"})
    sf = SuccessorFeatures(ag, {"input_layers": [N], "features": feats, "tau": 1.0, "eta": 0.01})
    w0 = np.array(sf.inputs[N.name]["w"]).copy()
    for t in range(T):
        ag.update(); N.update(); feats.update(); ff.update()
        sf.learn()
        if t == 0:                                         # one learn() step: no error, the weights moved
            torch.cuda.synchronize()
            w1 = np.array(sf.inputs[N.name]["w"])
            assert np.isfinite(w1).all() and np.abs(w1 - w0).max() > 0
    # FeedForwardLayer over the population's rows: W @ rates (+ bias) through the layer's activation, at the tolerance of
    # tests/test_gpu_parity.py's feed-forward tests
    ref, _ = orc.feedforward([N.firingrate], [ff.inputs[N.name]["w"]], ff.biases, {"activation": "linear"})
    assert np.allclose(ref, ff.inputs[N.name]["w"] @ N.firingrate + np.asarray(ff.biases).reshape(-1, 1))
    np.testing.assert_allclose(ff.firingrate, ref, rtol=2e-5, atol=2e-5)
    # rate maps
    gt, zero = N.get_rate_map(method="groundtruth")
    all_ = N.get_state(evaluate_at="all")
    assert not zero.any() and np.array_equal(gt, all_.reshape((17,) + tuple(env.discrete_coords.shape[:2])))
    maps, zero = N.get_rate_map(method="history")
    assert maps.shape[0] == 17 and maps.shape[1:] == zero.shape and not zero.all()
    assert np.isfinite(maps[:, ~zero]).all() and maps[:, ~zero].min() >= 0 and maps[:, ~zero].max() <= 1.0 + 1e-6


# ---- 8. the stream ABI ------------------------------------------------------------------------------------------------
def test_stream_supported_for_the_new_kind(riab):
    """riab_simulate asks stream_supported before anything is launched (the dry run of the row-following launch) and
    reports what it chose (riab_streamer_last_form): a single PlaneWaveNeurons population at B = 256 is the lead of the
    one-kernel form; with a noise state, or at B = 260, it is refused and the chunk form serves the run."""
    L = riab._lib
    for B, std, want in ((256, 0.0, "one-kernel"), (256, 0.1, "chunks"), (260, 0.0, "chunks")):
        np.random.seed(2)
        ag = riab.Agent(riab.Environment({}), {"n_agents": B, "dt": 0.01, "seed": 3})
        N = _PW()(ag, {"n": 8, "noise_std": std, "save_spikes": False})
        ag.simulate(8)
        torch.cuda.synchronize()
        assert ag.last_rate_stage_form() == want, (B, std)
        assert ag.engine_runs == {"native": 1, "plan": 0, "chunks": 0}
        assert N.get_history_tensors()[0].shape == (8, 8, ag._Bp)
    # the ABI by hand: kind 11 is accepted, 10 and 12 are no kinds — refused with nothing launched
    np.random.seed(2)
    ag = riab.Agent(riab.Environment({}), {"n_agents": 256, "dt": 0.01, "seed": 3})
    N = _PW()(ag, {"n": 8, "save_spikes": False})
    ag.simulate(4)
    torch.cuda.synchronize()
    env_s, _w = ag.Environment.device_tables(ag._device)
    m = ag._motion(ag.dt, False, 1, {})
    T = 8
    out = torch.empty((T, 8, ag._Bp), dtype=torch.float32, device="cuda")
    hist = torch.empty((T, L.HIST_ROWS, ag._Bp), dtype=torch.float32, device="cuda")

    def call(kind=None):
        arr = (L.RiabPopulation * 1)()
        L.C.memmove(L.C.byref(arr), L.C.byref(N._population()), L.C.sizeof(L.RiabPopulation))
        arr[0].rates_base, arr[0].spikes_base, arr[0].capacity_rows = out.data_ptr(), None, T
        if kind is not None:
            arr[0].kind = kind
        run = L.RiabSimulate()
        run.env, run.motion = L.C.pointer(env_s), L.C.pointer(m)
        run.state, run.B, run.agent_id0 = ag._state.data_ptr(), ag._Bp, 0
        run.seed, run.step0, run.T = int(ag.rng_seed), int(ag._step_index), T
        run.hist, run.diag, run.ctrl = hist.data_ptr(), ag._diag.data_ptr(), ag._ctrl.data_ptr()
        run.pops, run.n_pops, run.timed_pop = L.C.cast(arr, L.C.POINTER(L.RiabPopulation)), 1, -1
        return L.lib.riab_simulate(ag._streamer, L.C.byref(run), L.current_stream())

    before = ag.state_tensor.clone()
    assert call(kind=10) == L.EUNSUPPORTED and call(kind=12) == L.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(before, ag.state_tensor)
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(before, ag.state_tensor) and torch.isfinite(out).all()
