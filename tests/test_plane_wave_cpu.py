"""No-GPU checks of contribs.PlaneWaveNeurons: the float64 restatement of the reference's rule
(tests/plane_wave_oracle.py) is pinned to the reference's record (tests/golden/plane_wave_*.npz, written by
tests/golden/make_golden_plane_wave.py); the constructor's draws, the device table, the C ABI and what a step plan asks
of the new kind are checked the way tests/test_theta_cpu.py checks the phase-precessing place cells."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import golden_util as gu
from tests import plane_wave_oracle as pwo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "riab_hip.h")
FILES = sorted(f for f in os.listdir(gu.GOLDEN) if f.startswith("plane_wave_") and f.endswith(".npz"))


@pytest.fixture(scope="module")
def L():
    from ratinabox_amd import _lib
    return _lib


def _PW():
    from ratinabox_amd.contribs.PlaneWaveNeurons import PlaneWaveNeurons
    return PlaneWaveNeurons


def _cpu_population(g, **over):
    """The product's population of a golden file's configuration on a device="cpu" agent, seeded as the generator was."""
    import ratinabox_amd as riab
    env = riab.Environment({"boundary_conditions": "periodic" if bool(g["periodic"]) else "solid", "aspect": float(g["aspect"]),
                            "scale": float(g["scale"])})
    ag = riab.Agent(env, {"device": "cpu"})
    params = {"n": int(g["n"]), "wavescale": float(g["wavescale"]), "min_fr": float(g["min_fr"]), "max_fr": float(g["max_fr"])}
    params.update(over)
    np.random.seed(int(g["seed"]))
    return _PW()(ag, params)


# ---- the oracle --------------------------------------------------------------------------------------------------
def test_fixtures_cover_what_they_must():
    """Defaults, a periodic room with min_fr != 0, and hand-assigned arrays in a 2 x 1 m room with axis-aligned and
    diagonal w, wavelengths from 0.02 to 5 and offsets outside [0, lambda); corners, walls and the centre among the positions."""
    assert FILES == ["plane_wave_assigned.npz", "plane_wave_defaults.npz", "plane_wave_periodic.npz"]
    for name in FILES:
        g = gu.load(name)
        n, pos, ext = int(g["n"]), g["pos"], g["extent"]
        assert g["fr"].shape == (n, 256) and pos.shape == (256, 2) and g["w"].shape == (n, 2) and g["wavescales"].shape == (n,)
        np.testing.assert_allclose(np.linalg.norm(g["w"], axis=1), 1.0, rtol=1e-15)
        have = {(float(x), float(y)) for x, y in pos}
        for corner in ((ext[0], ext[2]), (ext[1], ext[2]), (ext[0], ext[3]), (ext[1], ext[3]), ((ext[0] + ext[1]) / 2, (ext[2] + ext[3]) / 2)):
            assert corner in have
        inside = lambda v, lo, hi: (v > lo) & (v < hi)   # noqa: E731
        for k, (axis, other) in enumerate(((0, 1), (0, 1), (1, 0), (1, 0))):
            wall = ext[2 * axis + k % 2]
            assert (((pos[:, axis] == wall) & inside(pos[:, other], ext[2 * other], ext[2 * other + 1])).sum()) >= 3
    d, p, a = (gu.load(f"plane_wave_{k}.npz") for k in ("defaults", "periodic", "assigned"))
    assert (int(d["n"]), float(d["wavescale"]), float(d["min_fr"]), float(d["max_fr"])) == (10, 0.2, 0.0, 1.0)
    assert bool(p["periodic"]) and (float(p["wavescale"]), float(p["min_fr"]), float(p["max_fr"])) == (0.05, 0.5, 10.0)
    assert list(a["extent"]) == [0.0, 2.0, 0.0, 1.0] and a["wavescales"].min() == 0.02 and a["wavescales"].max() == 5.0
    assert (np.abs(a["w"]) == 1).any() and (np.abs(np.abs(a["w"][:, 0]) - np.abs(a["w"][:, 1])) < 1e-15).any()
    assert (a["phase_offsets"] < 0).any() and (np.abs(a["phase_offsets"]).max(axis=1) > a["wavescales"]).any()


@pytest.mark.parametrize("name", FILES)
def test_oracle_equals_the_reference(name):
    """|oracle - reference| <= 1e-10 (max_fr - min_fr): a float64 cosine of a phase of at most about 2 pi 150 is good to
    about 1e3 2^-52 = 2e-13; four orders of margin."""
    g = gu.load(name)
    got = pwo.rates(g["pos"], g["phase_offsets"], g["w"], g["wavescales"], float(g["min_fr"]), float(g["max_fr"]))
    worst = float(np.abs(got - g["fr"]).max())
    fr_range = float(g["max_fr"]) - float(g["min_fr"])
    print(f"[{name}] worst |oracle - reference| = {worst:.2e} (allowed {1e-10 * fr_range:.1e})")
    assert got.shape == g["fr"].shape and worst <= 1e-10 * fr_range
    # ... and the revolutions form the device is handed says the same in float64
    tab = pwo.table(g["phase_offsets"], g["w"], g["wavescales"])
    rev = tab[:, :1] - (g["pos"][None, :, 0] * tab[:, 1:2] + g["pos"][None, :, 1] * tab[:, 2:3])
    alt = 0.5 * (np.cos(2 * np.pi * rev) + 1) * fr_range + float(g["min_fr"])
    assert np.abs(alt - g["fr"]).max() <= 1e-10 * fr_range


# ---- the class ---------------------------------------------------------------------------------------------------
def test_class_defaults_and_surface():
    import ratinabox_amd as riab
    from ratinabox_amd import contribs
    P = _PW()
    assert "PlaneWaveNeurons" in contribs.__all__
    assert P.default_params == {"n": 10, "wavescale": 0.2, "min_fr": 0, "max_fr": 1, "name": "PlaneWaveNeurons"}
    ag = riab.Agent(riab.Environment({}), {"n_agents": 3, "device": "cpu"})
    N = P(ag)
    assert isinstance(N, riab.Neurons) and N in ag.Neurons and (N.n, N.wavescale, N.name) == (10, 0.2, "PlaneWaveNeurons")
    assert N.phase_offsets.shape == (10, 2) and N.w.shape == (10, 2) and N.wavescales.shape == (10,)
    assert N._stream_kind == "plane_wave" and N._watch_arrays is None and not getattr(N, "_reads_agent_state", False)
    from ratinabox_amd.Neurons import FAST_REPEAT_TYPES
    assert P not in FAST_REPEAT_TYPES
    assert P.get_all_default_params()["noise_std"] == 0 and P.get_all_default_params()["wavescale"] == 0.2


def test_periodic_room_prints_the_notice(capsys):
    import ratinabox_amd as riab
    ag = riab.Agent(riab.Environment({"boundary_conditions": "periodic"}), {"device": "cpu"})
    _PW()(ag)
    assert "PlaneWaveNeurons not optimized for periodic environments" in capsys.readouterr().out
    ag = riab.Agent(riab.Environment({}), {"device": "cpu"})
    _PW()(ag)
    assert "PlaneWaveNeurons" not in capsys.readouterr().out


@pytest.mark.parametrize("name", ["plane_wave_defaults.npz", "plane_wave_periodic.npz"])
def test_constructor_draws_the_references_arrays(name):
    """The same draws in the same order: with the stored seed the three arrays are the reference's to the last bit."""
    g = gu.load(name)
    N = _cpu_population(g)
    for k in ("phase_offsets", "w", "wavescales"):
        got = np.asarray(getattr(N, k))
        assert got.dtype == np.float64 and got.shape == g[k].shape and np.array_equal(got, g[k]), k


@pytest.mark.parametrize("name", FILES)
def test_table_is_the_float64_formula_rounded_once(name, L):
    g = gu.load(name)
    N = _cpu_population(g)
    N.phase_offsets, N.w, N.wavescales = g["phase_offsets"].copy(), g["w"].copy(), g["wavescales"].copy()
    d = N._call(None, None)
    assert set(d) == {"kind", "table"} and d["kind"] == L.POP_KINDS["plane_wave"] == 11
    tab = d["table"].numpy()
    assert tab.shape == (int(g["n"]), 3) and tab.dtype == np.float32
    assert (tab[:, 0] >= 0).all() and (tab[:, 0] < 1).all()
    lam = g["wavescales"]
    a = (g["phase_offsets"] * g["w"]).sum(axis=1) / lam
    want = np.stack((a - np.floor(a), g["w"][:, 0] / lam, g["w"][:, 1] / lam), axis=-1).astype(np.float32)
    want[want[:, 0] >= 1, 0] = 0          # (a fraction that rounds up to 1.0f is the phase 0)
    assert np.array_equal(tab, want) and np.array_equal(tab, pwo.table32(g["phase_offsets"], g["w"], lam))
    # content-keyed: the same object while nothing changed, rebuilt after an in-place edit of any of the three arrays
    k0 = N._auto_key()
    assert N._call(None, None)["table"] is d["table"] and N._auto_key() == k0
    N.wavescales[3] *= 2
    k1 = N._auto_key()
    t1 = N._call(None, None)["table"]
    assert k1 != k0 and t1 is not d["table"]
    assert np.allclose(t1.numpy()[3, 1:], tab[3, 1:] / 2, rtol=1e-6) and np.array_equal(t1.numpy()[:3], tab[:3])
    N.w[0] = [0.0, 1.0]
    N.phase_offsets[1, 0] += 0.01
    assert N._auto_key() != k1 and N._call(None, None)["table"] is not t1
    pop = N._population({})
    assert (pop.kind, pop.n, pop.table) == (11, int(g["n"]), N._call(None, None)["table"].data_ptr())
    assert (pop.io.min_fr, pop.io.max_fr) == (float(g["min_fr"]), float(g["max_fr"])) and not pop.noise_state


# ---- the C ABI ---------------------------------------------------------------------------------------------------
def test_abi_symbol_kind_and_version(L):
    src = open(HEADER).read()
    assert hasattr(L.lib, "riab_plane_wave_neurons") and "riab_plane_wave_neurons" in L.PROTOTYPES
    assert re.search(r"\bint riab_plane_wave_neurons\(const RiabRateIO\* io, const float\* table, int32_t n,\s*riab_stream_t stream\);", src)
    assert re.search(r"RIAB_POP_PLANE_WAVE = (\d+)", src).group(1) == str(L.POP_KINDS["plane_wave"]) == "11"
    assert 10 not in L.POP_KINDS.values() and not re.search(r"RIAB_POP_\w+ = 10\b", src)
    # purely additive: the version and the population struct are the parent's
    assert int(re.search(r"#define RIAB_ABI_VERSION (\d+)", src).group(1)) == L.ABI_VERSION == L.lib.riab_abi_version() == 11
    assert L.lib.riab_abi_sizeof(3) == C.sizeof(L.RiabPopulation) and L.RiabPopulation._fields_[-1][0] == "kappa"
    assert "riab_plane_wave_neurons" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_plan_add_asks_for_the_table_and_ten_stays_refused(L):
    env, m = L.RiabEnv(), L.RiabMotion()
    m.dt = 0.001
    h = L.lib.riab_plan_create(env, m, C.c_void_p(64), 4, 0, 7, 5, C.c_void_p(64), None)
    assert h
    pop = L.RiabPopulation()
    pop.kind, pop.n = L.POP_KINDS["plane_wave"], 4
    assert L.lib.riab_plan_add(h, pop) == L.EINVAL                          # no table
    pop.table = 64
    assert L.lib.riab_plan_add(h, pop) == 0
    assert L.lib.riab_plan_add(h, pop) == 1
    pop.n = 0
    assert L.lib.riab_plan_add(h, pop) == L.EINVAL
    pop.n = 4
    for kind in (10, 12, -1):
        pop.kind = kind
        assert L.lib.riab_plan_add(h, pop) == L.EINVAL, kind
    L.lib.riab_plan_destroy(h)


def _io(L, **over):
    io = L.RiabRateIO()
    io.pos_x = io.pos_y = io.rates = 64
    io.T, io.B, io.pos_ld = 1, 8, 8
    for k, v in over.items():
        setattr(io, k, v)
    return io


def test_argument_errors_before_launch(L):
    """Negative codes come from validation only (riab_grid_cells' checks): no device needed, nothing is launched."""
    f, tab = L.lib.riab_plane_wave_neurons, C.c_void_p(64)
    assert f(None, tab, 4, None) == L.EINVAL
    assert f(_io(L), None, 4, None) == L.EINVAL
    assert f(_io(L), tab, 0, None) == L.EINVAL and f(_io(L), tab, -3, None) == L.EINVAL
    assert f(_io(L, pos_x=None), tab, 4, None) == L.EINVAL and f(_io(L, pos_y=None), tab, 4, None) == L.EINVAL
    assert f(_io(L, rates=None), tab, 4, None) == L.EINVAL and f(_io(L, T=0), tab, 4, None) == L.EINVAL
    assert f(_io(L, B=6), tab, 4, None) == L.EALIGN and f(_io(L, rates=68), tab, 4, None) == L.EALIGN
    assert f(_io(L, u_in=64), tab, 4, None) == L.EINVAL                     # explicit uniforms without a spike buffer
