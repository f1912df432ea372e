"""What tests/vector_edge_cases.py claims about its own cases, checked with the oracle alone (no GPU): the narrow tunings
have populated peaks, the occlusion decisions are nowhere near a tie, the periodic room does wrap, the degenerate
geometry is finite — so that tests/test_gpu_vector_edges.py cannot pass vacuously — and the host-side refusals that
need no device."""
import numpy as np
import pytest

from oracle import riab_oracle as orc
from tests import vector_edge_cases as vc


def _f32_exact(*arrays):
    return all(np.array_equal(a, a.astype(np.float32).astype(np.float64)) for a in arrays)


@pytest.mark.parametrize("ego", [False, True])
@pytest.mark.parametrize("width", vc.WIDTHS)
def test_narrow_ovc_cases_populate_the_peaks(width, ego):
    c = vc.narrow_ovc(width, ego)
    assert _f32_exact(c["pos"], c["hd"], c["objects"])
    assert c["pos"].shape == (257, 2) and len(c["mu_d"]) == 24 and len(c["objects"]) == 5
    assert len(np.unique(c["object_types"])) == 2 and np.allclose(np.degrees(c["sg_t"]), width)
    assert c["pos"].min() > 0 and c["pos"].max() < 1
    for occlude in (False, True):
        ref = vc.ovc_reference(c, occlude, ego)
        assert ref.shape == (24, 257) and np.isfinite(ref).all()
        assert (ref > 0.01).sum() >= 50, (width, ego, occlude, int((ref > 0.01).sum()))
    # the occlusion is not a formality: the two walls hide something, and not everything
    hidden = vc.ovc_reference(c, False, ego) != vc.ovc_reference(c, True, ego)
    assert 0 < hidden.mean() < 0.9
    # the case is deterministic
    assert np.array_equal(vc.narrow_ovc(width, ego)["pos"], c["pos"])


def test_manifold_cases():
    tuning = vc.uniform_manifold()
    assert len(tuning[0]) == 498
    assert np.degrees(tuning[3].min()) < 3.1 and np.degrees(tuning[3].min()) > 2.9
    c = vc.manifold_case(tuning)
    assert _f32_exact(c["pos"], c["pos_avc"], c["hd"], c["other"], c["objects"])
    for ref in (vc.ovc_reference(c, True, True), vc.avc_reference(c)):
        assert ref.shape == (498, 257) and (ref > 0.01).sum() >= 50
        assert (ref[tuning[3] < np.radians(3.1)] > 0.01).sum() >= 1      # the narrowest cells do fire
    narrow = tuple(np.array(v) for v in (tuning[0][:40], tuning[1][:40], tuning[2][:40], np.full(40, np.radians(3.0))))
    c3 = vc.manifold_case(narrow, seed=44)
    assert (vc.avc_reference(c3) > 0.01).sum() >= 50


@pytest.mark.parametrize("width", vc.WIDTHS)
def test_narrow_direction_cases_populate_the_peaks(width):
    hd = vc.narrow_directions(width)
    assert _f32_exact(hd) and hd.shape == (257, 2)
    ref = orc.head_direction_cells(hd, vc.HD_N, width)
    assert (ref > 0.01).sum() >= 50 and (ref > 0.5).sum() >= 50
    v = vc.narrow_directions(width, speeds=True)
    ref = orc.velocity_cells(v, vc.HD_N, 0.16, width)
    assert _f32_exact(v) and (ref > 0.01).sum() >= 50


def test_lds_regimes_are_the_ones_the_counts_name():
    per = vc.LDS_PER_OBJECT
    assert per == 768
    assert 85 * per <= vc.LDS_DEFAULT < 86 * per          # the last count that needs no raised limit, the first that does
    assert 213 * per <= vc.LDS_CU < 214 * per             # the last count a CU can hold, the first it cannot
    assert {85, 86, 213} <= set(vc.OBJECT_COUNTS) and min(vc.REFUSED_COUNTS) == 214


@pytest.mark.parametrize("M", vc.OBJECT_COUNTS)
def test_many_object_cases(M):
    c = vc.many_objects(M)
    assert _f32_exact(c["pos"], c["hd"], c["objects"], c["walls"]) and len(c["walls"]) == 12
    types, tt = c["object_types"], c["ttypes"]
    # add_object accepts the types in this order; type 1 has a single object, no cell prefers type 2
    seen = 0
    for t in types:
        assert t <= seen
        seen = max(seen, t + 1)
    if M >= 2:
        assert (types == 1).sum() == 1 and (tt == 1).sum() == 1
    if M >= 4:
        counts = np.bincount(types)
        assert len(counts) == 3 and len(set(counts)) == 3 or M < 6
        assert (types == 2).any() and not (tt == 2).any()
    for n in vc.CELL_COUNTS:
        assert len(vc.tuning_types_for(n)) == n and not (vc.tuning_types_for(n) == 2).any()
    # the per-object terms ARE what the oracle sums
    for ego in (False, True):
        terms = vc.ovc_terms(c, True, ego)
        ref = vc.ovc_reference(c, True, ego)
        np.testing.assert_allclose(terms.sum(axis=1).T, ref, rtol=1e-13, atol=1e-300)
        assert vc.sum_allowance(terms).shape == ref.shape
        assert (vc.sum_allowance(terms) <= M * 2.0 ** -24 * np.abs(ref) * (1 + 1e-12)).all()   # positive terms: M eps |ref|
    # no line of sight is near a tie with a wall; a fair share is blocked, a fair share is not
    margin, blocked = vc.occlusion_margins(c)
    assert margin.min() > 1e-9, margin.min()               # (nothing excluded: the budget of 0.1% of positions is unused)
    assert np.array_equal(blocked, orc.env_distances(orc.EnvSpec(walls=c["walls"]), c["pos"], c["objects"], "line_of_sight") == 1000.0)
    if M >= 5:
        assert 0.2 <= blocked.mean() <= 0.9, blocked.mean()
    for P in vc.POSITION_COUNTS:
        small = vc.many_objects(M, n=3, P=P)
        assert np.array_equal(small["pos"], c["pos"][:P]) and np.array_equal(small["mu_d"], c["mu_d"][:3])


def test_periodic_case_wraps():
    c = vc.periodic_case()
    s = vc.PERIODIC["scale"]
    assert _f32_exact(c["pos"], c["hd"], c["objects"], c["other"])
    for targets in (c["objects"], c["other"]):
        edge = np.minimum(np.minimum(targets[:, 0], 1.6 * s - targets[:, 0]), np.minimum(targets[:, 1], s - targets[:, 1]))
        assert (edge <= 0.1 * s).all() and (edge > 0).all()
        wrapped, clear = vc.wrap_report(c, targets)
        assert wrapped >= 0.2 and clear > 1e-6, (wrapped, clear)
    env = vc.periodic_env()
    assert env.periodic and len(env.walls) == 0
    ref = vc.ovc_reference(c, False, True, env=env)
    flat = vc.ovc_reference(c, False, True, env=orc.EnvSpec(boundary_conditions="solid", **vc.PERIODIC))
    assert (ref > 0.01).sum() >= 50 and (np.abs(ref - flat) > 0.01).sum() >= 50     # the wrap changes the answer
    assert (vc.avc_reference(c, walls_occlude=False, env=env) > 0.01).sum() >= 50


def test_degenerate_case_is_finite():
    c = vc.degenerate_case()
    d = np.linalg.norm(c["pos"][:, None] - c["objects"][None], axis=-1)
    assert (d.min(axis=1) == 0).sum() == 16 and (np.abs(c["hd"]).sum(axis=1) == 0).sum() == 16
    assert orc.get_angle(np.zeros(2)) == 0.0
    for ego in (False, True):
        ref = vc.ovc_reference(c, False, ego)
        assert np.isfinite(ref).all() and (ref[:, 0::4] > 0.01).any()


def test_periodic_occlusion_is_refused_without_a_device():
    """`walls_occlude=True` in a periodic room: the reference refuses it (line_of_sight geometry needs solid boundaries),
    and so does the C entry point, before anything is launched."""
    import ctypes as C
    import ratinabox_amd as riab
    L = riab._lib
    env = L.RiabEnv()
    env.periodic, env.scale, env.n_walls = 1, 0.8, 0
    io = L.RiabRateIO()
    io.T, io.B, io.pos_ld = 1, 4, 4
    dummy = C.c_void_p(64)
    io.pos_x = io.pos_y = io.hd_x = io.hd_y = io.rates = 64     # never dereferenced: the call returns before any launch
    rc = L.lib.riab_object_vector_cells(env, io, dummy, dummy, 1, dummy, 1, 1, 0, None)
    assert rc == L.EUNSUPPORTED
    assert L.lib.riab_agent_vector_cells(env, io, dummy, dummy, 0, dummy, 1, 1, 0, None) == L.EUNSUPPORTED
