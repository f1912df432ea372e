"""No-GPU checks of contribs.PhasePrecessingPlaceCells: the float64 restatement of the reference's rule
(tests/theta_oracle.py) is pinned to the reference's record (tests/golden/theta_*.npz, written by
tests/golden/make_golden_theta.py), and the C ABI and the class surface are checked the way tests/test_abi_cpu.py and
tests/test_td_cpu.py check the rest."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import golden_util as gu
from tests import theta_oracle as tho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "riab_hip.h")
SETS = sorted(f for f in os.listdir(gu.GOLDEN) if f.startswith("theta_set_") and f.endswith(".npz"))


@pytest.fixture(scope="module")
def L():
    from ratinabox_amd import _lib
    return _lib


# ---- the oracle --------------------------------------------------------------------------------------------------
def test_fixtures_cover_what_they_must():
    """Four descriptions, solid and periodic rooms, min_fr != 0, kappa 1 / 2 / 4; per configuration time stamps on both
    sides of a multiple of the theta period, points beside walls, resting agents."""
    assert len(SETS) >= 6
    seen = set()
    for name in SETS:
        g = gu.load(name)
        seen.add((str(g["description"]), bool(g["periodic"])))
        seen.add(("kappa", float(g["kappa"])))
        seen.add(("min_fr != 0", float(g["min_fr"]) != 0))
        t, tf = g["t"], float(g["theta_freq"])
        th = np.array([tho.theta_rev(x, tf) for x in t])
        assert len(t) >= 16 and g["pos"].shape[0] >= 256 and g["fr"].shape == (len(t), len(g["pos"]), len(g["centres"]))
        assert (th > 0.999).any() and ((th < 0.001) & (t > 0)).any()           # just before / just after a wrap
        assert (np.linalg.norm(g["vel"], axis=1) == 0).sum() >= 4
        d_wall = np.minimum(g["pos"], 1 - g["pos"]).min(axis=1)
        assert (d_wall < 0.02).sum() >= 16
    assert {d for d, _p in seen if d in tho.DESCRIPTIONS} == set(tho.DESCRIPTIONS)
    assert {p for d, p in seen if d in tho.DESCRIPTIONS} == {False, True}
    assert {("kappa", 1.0), ("kappa", 2.0), ("kappa", 4.0), ("min_fr != 0", True)} <= seen


@pytest.mark.parametrize("name", SETS)
def test_oracle_equals_the_reference_on_set_state_samples(name):
    g = gu.load(name)
    cfg = tho.config_of(g)
    worst = 0.0
    for k, t in enumerate(g["t"]):
        got = tho.rates(g["pos"], g["vel"], t, **cfg).T
        worst = max(worst, float(np.abs(got - g["fr"][k]).max()))
    print(f"[{name}] worst |oracle - reference| = {worst:.2e}")
    assert worst <= 1e-12


def test_oracle_equals_the_reference_on_the_rollout():
    """... and the rollout pins WHICH velocity and clock update() reads: Agent.velocity (not the measured velocity, which
    differs beside the wall the run starts at) and t after the agent's update."""
    g = gu.load("theta_rollout.npz")
    cfg = tho.config_of(g)
    T = len(g["t"])
    assert T >= 2000 and abs(float(g["dt"]) - 1e-3) < 1e-15
    worst, worst_measured, worst_prev_t = 0.0, 0.0, 0.0
    for k in range(T):
        got = tho.rates(g["pos"][k], g["vel"][k], g["t"][k], **cfg)[:, 0]
        worst = max(worst, float(np.abs(got - g["fr"][k]).max()))
        other = tho.rates(g["pos"][k], g["mvel"][k], g["t"][k], **cfg)[:, 0]
        worst_measured = max(worst_measured, float(np.abs(other - g["fr"][k]).max()))
        late = tho.rates(g["pos"][k], g["vel"][k], g["t"][k] - float(g["dt"]), **cfg)[:, 0]
        worst_prev_t = max(worst_prev_t, float(np.abs(late - g["fr"][k]).max()))
    print(f"[rollout] worst |oracle - reference| = {worst:.2e}; with the measured velocity {worst_measured:.2e}; "
          f"with the clock before the update {worst_prev_t:.2e}")
    assert worst <= 1e-12
    assert worst_measured > 1e-3 and worst_prev_t > 1e-3


def test_modulation_comes_after_the_affine_map():
    """Far from every field the rate is min_fr * M, not min_fr."""
    cfg = dict(centres=np.array([[0.1, 0.1]]), widths=0.02, description="gaussian_threshold", theta_freq=10.0, kappa=2.0,
               precess_fraction=0.5)
    pos, vel, t = np.array([[0.9, 0.9]]), np.array([[0.1, 0.0]]), 0.0123
    M = tho.modulation(pos, vel, t, **cfg)
    r = tho.rates(pos, vel, t, min_fr=0.5, max_fr=3.0, **cfg)
    np.testing.assert_allclose(r, 0.5 * M, rtol=1e-15)
    assert abs(M[0, 0] - 1) > 0.05
    # at rest the preferred phase is pi whatever the position
    M0 = tho.modulation(pos, np.zeros((1, 2)), t, **cfg)
    expect = np.exp(2.0 * (np.cos(2 * np.pi * (0.5 - 0.123)) - 1)) * tho.von_mises_peak(2.0)
    np.testing.assert_allclose(M0[0, 0], expect, rtol=1e-13)


def test_float32_run_of_the_oracle_is_close():
    """The same text in np.float32: its error against the reference is what the device's allowance is derived from;
    it has to be a small multiple of the project's bound for that derivation to mean anything."""
    for name in SETS:
        g = gu.load(name)
        cfg = tho.config_of(g)
        c = max(tho.ratio(tho.rates(g["pos"], g["vel"], t, dtype=np.float32, **cfg).T, g["fr"][k], cfg["max_fr"] - cfg["min_fr"])
                for k, t in enumerate(g["t"]))
        print(f"[{name}] float32 oracle: worst |err| / (1e-5 (|ref| + range)) = {c:.3f}")
        assert 0 < c < 4


# ---- the C ABI ---------------------------------------------------------------------------------------------------
def test_abi_version_symbols_and_population_mirror(L):
    src = open(HEADER).read()
    assert int(re.search(r"#define RIAB_ABI_VERSION (\d+)", src).group(1)) == L.ABI_VERSION >= 10
    assert L.lib.riab_abi_version() == L.ABI_VERSION
    for s in ("riab_phase_precessing_place_cells", "riab_plan_set_clock", "riab_plan_clock"):
        assert hasattr(L.lib, s) and s in L.PROTOTYPES and re.search(r"\b%s\(" % s, src), s
    assert re.search(r"RIAB_POP_THETA_PLACE = (\d+)", src).group(1) == str(L.POP_KINDS["theta_place"])
    body = re.search(r"typedef struct RiabPopulation \{(.*?)\} RiabPopulation;", src, re.S).group(1)
    names = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+)(?:\[[^\]]*\])?;", body, re.M)
    assert names == [f[0] for f in L.RiabPopulation._fields_]
    assert names[-2:] == ["theta_freq", "kappa"]
    assert L.lib.riab_abi_sizeof(3) == C.sizeof(L.RiabPopulation) == L.POP_SIZE
    P = L.RiabPopulation
    assert P.theta_freq.offset % 8 == 0 and P.kappa.offset == P.theta_freq.offset + 8 == C.sizeof(P) - 8


def _io(L, **over):
    io = L.RiabRateIO()
    io.pos_x = io.pos_y = io.rates = 64
    io.T, io.B, io.pos_ld = 1, 8, 8
    for k, v in over.items():
        setattr(io, k, v)
    return io


def test_argument_errors_before_launch(L):
    """Negative codes come from validation only: no device needed.  The checks are riab_velocity_cells' (T == 1 with the
    state velocity, 32-byte aligned rows) and riab_place_cells' (the io block), plus the descriptions and geometries."""
    env, ok, tab = L.RiabEnv(), C.c_void_p(64), C.c_void_p(64)
    f = L.lib.riab_phase_precessing_place_cells

    def call(io=None, env=env, tab=tab, n=4, desc=0, geom=0, kappa=1.0, theta=0.25, vx=ok, vy=ok):
        return f(env, _io(L) if io is None else io, tab, n, desc, geom, 0.2, kappa, theta, vx, vy, None)

    assert call(env=None) == L.EINVAL and call(tab=None) == L.EINVAL and call(n=0) == L.EINVAL
    assert f(env, None, tab, 4, 0, 0, 0.2, 1.0, 0.25, ok, ok, None) == L.EINVAL
    assert call(vx=None) == L.EINVAL and call(vy=None) == L.EINVAL and call(vx=None, vy=None) == L.EINVAL   # no history-row form
    assert call(kappa=-1.0) == L.EINVAL and call(kappa=float("nan")) == L.EINVAL and call(theta=float("nan")) == L.EINVAL
    assert call(_io(L, pos_x=None)) == L.EINVAL and call(_io(L, rates=None)) == L.EINVAL
    assert call(_io(L, T=2)) == L.EINVAL                                   # the state holds the current step only
    assert call(_io(L, B=6)) == L.EALIGN and call(_io(L, rates=68)) == L.EALIGN
    assert call(vx=C.c_void_p(80)) == L.EALIGN and call(vy=C.c_void_p(72)) == L.EALIGN     # 16- / 8-byte aligned: not enough
    assert call(desc=L.PC_DESCRIPTIONS["one_hot"]) == L.EINVAL and call(desc=17) == L.EINVAL
    assert call(geom=L.GEOMETRIES["line_of_sight"]) == L.EUNSUPPORTED
    assert call(geom=L.GEOMETRIES["geodesic"]) == L.EUNSUPPORTED and call(geom=9) == L.EINVAL
    periodic = L.RiabEnv()
    periodic.periodic = 1
    assert call(env=periodic, geom=L.GEOMETRIES["geodesic"]) == L.EUNSUPPORTED


def test_plan_clock_and_population_kind(L):
    """riab_plan_set_clock / riab_plan_clock and what riab_plan_add asks of the new kind, before any launch."""
    env, m = L.RiabEnv(), L.RiabMotion()
    m.dt = 0.001
    h = L.lib.riab_plan_create(env, m, C.c_void_p(64), 4, 0, 7, 5, C.c_void_p(64), None)
    assert h
    assert L.lib.riab_plan_clock(h) == 0.0
    assert L.lib.riab_plan_set_clock(h, 1.25) == 0 and L.lib.riab_plan_clock(h) == 1.25
    assert L.lib.riab_plan_set_clock(h, float("nan")) == L.EINVAL and L.lib.riab_plan_set_clock(None, 0.0) == L.EINVAL
    pop = L.RiabPopulation()
    pop.kind, pop.n = L.POP_KINDS["theta_place"], 4
    assert L.lib.riab_plan_add(h, pop) == L.EINVAL                          # no table
    pop.table = 64
    assert L.lib.riab_plan_add(h, pop) == L.EINVAL                          # theta_freq must be positive
    pop.theta_freq, pop.kappa = 10.0, -1.0
    assert L.lib.riab_plan_add(h, pop) == L.EINVAL
    pop.kappa = 2.0
    assert L.lib.riab_plan_add(h, pop) == 0
    pop.kind = L.POP_KINDS["theta_place"] + 1
    assert L.lib.riab_plan_add(h, pop) == L.EINVAL
    L.lib.riab_plan_destroy(h)


# ---- the class ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def cpu_agent():
    import ratinabox_amd as riab
    np.random.seed(0)
    return riab, riab.Agent(riab.Environment({}), {"n_agents": 3, "device": "cpu"})


def test_class_defaults_assertion_and_sigma(cpu_agent):
    riab, ag = cpu_agent
    from ratinabox_amd.contribs.PhasePrecessingPlaceCells import PhasePrecessingPlaceCells
    P = PhasePrecessingPlaceCells
    assert P.default_params == {"n": 10, "min_fr": 0, "max_fr": 1, "theta_freq": 10, "kappa": 1, "precess_fraction": 0.5,
                                "description": "gaussian_threshold", "name": "PhasePrecessingPlaceCell"}
    N = P(ag)
    assert isinstance(N, riab.PlaceCells) and N in ag.Neurons
    assert (N.n, N.theta_freq, N.kappa, N.precess_fraction, N.description, N.name) == (10, 10, 1, 0.5, "gaussian_threshold",
                                                                                        "PhasePrecessingPlaceCell")
    assert N.widths == 0.2 and N.wall_geometry == "geodesic" and N.place_cell_centres.shape == (10, 2)   # PlaceCells' own defaults
    assert P(ag, {"kappa": 4}).sigma == 0.5 and N.sigma == 1.0
    with pytest.raises(AssertionError):
        P(ag, {"description": "one_hot"})
    all_params = P.get_all_default_params()
    assert all_params["theta_freq"] == 10 and all_params["widths"] == 0.2 and all_params["noise_std"] == 0
    assert N._reads_agent_state and N._stream_kind is None and N._state_op is None
    for k in ("theta_freq", "kappa", "precess_fraction"):
        assert k in P._watch_scalars
    with pytest.raises(NotImplementedError, match="step plan"):
        N._rates_from_trajectory(None, None, 0, 1, 0, 0.01, None)


def test_theta_modulation_factors_is_the_oracle(cpu_agent):
    riab, ag = cpu_agent
    from ratinabox_amd.contribs.PhasePrecessingPlaceCells import PhasePrecessingPlaceCells
    for desc in ("gaussian", "top_hat"):
        N = PhasePrecessingPlaceCells(ag, {"n": 7, "description": desc, "kappa": 2, "theta_freq": 8, "precess_fraction": 0.75})
        ag.t = 0.4321
        ag.velocity = np.array([[0.1, 0.02], [0.0, 0.0], [-0.03, 0.2]])
        got = N.theta_modulation_factors()
        ref = tho.modulation(ag.pos, ag.velocity, ag.t, N.place_cell_centres, N.place_cell_widths, desc, 8, 2, 0.75)
        assert got.shape == (7, 3)
        np.testing.assert_allclose(got, ref, rtol=1e-13)
    one = riab.Agent(riab.Environment({}), {"device": "cpu"})
    assert PhasePrecessingPlaceCells(one, {"n": 5}).theta_modulation_factors().shape == (5,)


def test_descriptor_follows_in_place_edits(cpu_agent):
    """What a step plan / the automatic stepper records of the population is keyed on content: the table on the
    centres, widths, description and precess_fraction; theta_freq and kappa by value."""
    riab, ag = cpu_agent
    from ratinabox_amd.contribs.PhasePrecessingPlaceCells import PhasePrecessingPlaceCells
    from ratinabox_amd import _lib as L
    N = PhasePrecessingPlaceCells(ag, {"n": 6, "description": "gaussian", "widths": 0.25})
    d0, k0 = N._call(None, None), N._auto_key()
    assert d0["kind"] == L.POP_KINDS["theta_place"] and d0["table"].shape == (6, 4) and N._auto_key() == k0
    tab = d0["table"].numpy().astype(np.float64)
    np.testing.assert_allclose(tab[:, :2], N.place_cell_centres, rtol=1e-7)
    np.testing.assert_allclose(tab[:, 2], -np.log2(np.e) / (2 * 0.25 ** 2), rtol=1e-7)
    np.testing.assert_allclose(tab[:, 3], 0.5 / (2 * 2 * 0.25), rtol=1e-7)      # gaussian: the boundary at two widths
    assert N._call(None, None)["table"] is d0["table"]
    N.kappa = 4
    assert N._auto_key() != k0 and N._call(None, None)["kappa"] == 4.0 and N._call(None, None)["table"] is d0["table"]
    N.theta_freq = 5
    assert N._call(None, None)["theta_freq"] == 5.0
    N.precess_fraction = 1.0
    t1 = N._call(None, None)["table"]
    assert t1 is not d0["table"] and abs(float(t1[0, 3]) - 1.0) < 1e-6
    N.place_cell_centres[-1] = [0.9, 0.9]
    assert N._call(None, None)["table"] is not t1
    pop = N._population({})
    assert (pop.kind, pop.theta_freq, pop.kappa, pop.n) == (L.POP_KINDS["theta_place"], 5.0, 4.0, 6)
    N.wall_geometry = "line_of_sight"
    with pytest.raises(NotImplementedError, match="euclidean"):
        N._call(None, None)
