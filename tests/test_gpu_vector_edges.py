"""csrc/riab_ovc.hip (ObjectVectorCells, AgentVectorCells, the field-of-view manifolds) and HDCell::eval
(HeadDirectionCells, VelocityCells) at the edges tests/vector_edge_cases.py builds, against oracle.riab_oracle
(tests/test_vector_edges_cpu.py checks what the cases claim about themselves):

A. angular widths of 30, 10, 5, 3 and 1 degrees with the peaks populated, where `kappa (cos - 1)` cancels;
B. 1 .. 213 objects through the LDS regimes of the launch (default, raised limit), 214 and more refused;
C. a periodic room;
D. objects added under a live population, an object at the position, a head direction of (0, 0).

The check is the project's own with the floor on, |got - ref| <= 1e-5 |ref| + 1e-5 (max_fr - min_fr), plus, where many
objects are summed, M 2^-24 sum |term| from the oracle's own terms.  Every worst err / tol is printed (docs/EXPERIMENTS.md
records them)."""
import numpy as np
import pytest
import torch

from oracle import riab_oracle as orc
from tests import vector_edge_cases as vc

pytestmark = pytest.mark.gpu

f32 = vc.f32


@pytest.fixture(scope="module")
def riab():
    assert torch.cuda.is_available(), "these tests need the GPU"
    import ratinabox_amd
    return ratinabox_amd


def check(what, got, ref, scale=1.0, extra=0.0):
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    ratio = np.abs(got - ref) / vc.tolerance(ref, scale, extra)
    worst = float(ratio.max())
    print(f"vector-edges {what}: worst err/tol {worst:.3f} ({int((ratio > 1).sum())} of {ratio.size} outside)")
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} / {ratio.size} outside tolerance, worst err/tol {worst:.3f}"
    return worst


def make_env(riab, c, **kw):
    env = riab.Environment(dict(walls=np.asarray(c["walls"]).tolist(), **kw))
    for o, t in zip(c["objects"], c["object_types"]):
        env.add_object(o, type=int(t))
    assert np.array_equal(env.objects["object_types"], c["object_types"])
    return env


def tune(N, c):
    n = int(N.n)
    assert n == len(c["mu_d"])
    N.tuning_distances, N.tuning_angles = np.array(c["mu_d"]), np.array(c["mu_t"])
    N.sigma_distances, N.sigma_angles = np.array(c["sg_d"]), np.array(c["sg_t"])
    return N


def make_ovc(riab, Ag, c, ego, occlude, **kw):
    prm = dict(n=len(c["mu_d"]), reference_frame="egocentric" if ego else "allocentric", walls_occlude=occlude,
               object_tuning_type=[int(x) for x in c["ttypes"]], **kw)
    return tune(riab.ObjectVectorCells(Ag, prm), c)


def ovc_state(O, c, ego):
    return O.get_state(evaluate_at=None, pos=c["pos"], **(dict(head_direction=c["hd"]) if ego else {}))


# ----------------------------------------------------------------------------- A. narrow angular tunings
@pytest.mark.parametrize("ego", [False, True], ids=["allo", "ego"])
@pytest.mark.parametrize("width", vc.WIDTHS)
def test_narrow_object_vector_cells(riab, width, ego):
    c = vc.narrow_ovc(width, ego)
    Ag = riab.Agent(make_env(riab, c))
    for occlude in (False, True):
        O = make_ovc(riab, Ag, c, ego, occlude)
        check(f"ovc {width:g}deg {'ego' if ego else 'allo'} occlude={occlude}", ovc_state(O, c, ego),
              vc.ovc_reference(c, occlude, ego))


def _two_agents(riab, env, c):
    P = len(c["pos_avc"])
    A, B = riab.Agent(env, {"n_agents": P}), riab.Agent(env, {"n_agents": P})
    A.pos, B.pos, A.head_direction = c["pos_avc"], c["other"], c["hd"]
    return A, B


def test_uniform_manifold_field_of_view_cells(riab):
    """FieldOfViewOVCs / FieldOfViewAVCs on the uniform manifold at the reference's default ranges: 498 cells, angular
    sigmas down to 3.02 degrees; AgentVectorCells with every angular sigma set to 3 degrees."""
    c = vc.manifold_case(vc.uniform_manifold())
    env = make_env(riab, c)
    Ag = riab.Agent(env)
    O = riab.FieldOfViewOVCs(Ag, {"cell_arrangement": "uniform_manifold", "object_tuning_type": 0})
    assert O.n == 498 and np.degrees(np.min(O.sigma_angles)) < 3.1
    for k, v in (("tuning_distances", "mu_d"), ("tuning_angles", "mu_t"), ("sigma_distances", "sg_d"), ("sigma_angles", "sg_t")):
        assert np.array_equal(getattr(O, k), c[v])
    check("fov ovc uniform manifold", ovc_state(O, c, True), vc.ovc_reference(c, True, True))
    A, B = _two_agents(riab, riab.Environment(), c)
    N = riab.FieldOfViewAVCs(A, B, {"cell_arrangement": "uniform_manifold"})
    assert N.n == 498 and np.array_equal(N.sigma_angles, c["sg_t"])
    N.update()
    check("fov avc uniform manifold", N.firingrate, vc.avc_reference(c))
    t = vc.uniform_manifold()
    c3 = vc.manifold_case((t[0][:40], t[1][:40], t[2][:40], np.full(40, np.radians(3.0))), seed=44)
    A, B = _two_agents(riab, riab.Environment(), c3)
    N3 = tune(riab.AgentVectorCells(A, B, {"n": 40, "reference_frame": "egocentric"}), c3)
    N3.update()
    check("avc 3deg", N3.firingrate, vc.avc_reference(c3))


@pytest.mark.parametrize("width", vc.WIDTHS)
def test_narrow_head_direction_cells_get_state(riab, width):
    hd = vc.narrow_directions(width)
    Ag = riab.Agent(riab.Environment(), {"n_agents": len(hd)})
    H = riab.HeadDirectionCells(Ag, {"n": vc.HD_N, "angular_spread_degrees": width, "min_fr": 0.5, "max_fr": 4.5})
    ref = orc.head_direction_cells(hd, vc.HD_N, width, min_fr=0.5, max_fr=4.5)
    check(f"hdc {width:g}deg get_state(pos=)", H.get_state(evaluate_at=None, pos=np.zeros_like(hd), head_direction=hd), ref, scale=4.0)
    Ag.head_direction = hd                  # at the agents: the float64 state, rounded to fp32 by the launch
    check(f"hdc {width:g}deg get_state()", H.get_state(), ref, scale=4.0)
    H.update()
    check(f"hdc {width:g}deg update()", H.firingrate, ref, scale=4.0)


def test_narrow_velocity_cells_get_state(riab):
    v = vc.narrow_directions(3.0, speeds=True)
    Ag = riab.Agent(riab.Environment(), {"n_agents": len(v), "speed_mean": 0.15})
    V = riab.VelocityCells(Ag, {"n": vc.HD_N, "angular_spread_degrees": 3.0})
    Ag.velocity = v
    ref = orc.velocity_cells(v, vc.HD_N, V.one_sigma_speed, 3.0)
    assert (ref > 0.01).sum() >= 50
    check("velocity 3deg get_state()", V.get_state(), ref)
    V.update()
    check("velocity 3deg update()", V.firingrate, ref)


def _stepping_paths(riab, cls, prm, oracle, T=12, B=70):
    """The eager loop against the oracle at every step; a step plan and Agent.simulate() reproduce it bit for bit."""
    def world():
        np.random.seed(11)
        Ag = riab.Agent(riab.Environment(), {"n_agents": B, "dt": 0.05, "speed_mean": 0.2, "seed": 9})
        return Ag, cls(Ag, dict(prm))

    Ag, N = world()
    worst, peaks = 0.0, 0
    for t in range(T):
        Ag.update()
        N.update()
        ref = oracle(Ag, N)
        peaks += int((ref > 0.25).sum())
        worst = max(worst, check(f"{cls.__name__} {prm['angular_spread_degrees']:g}deg step {t}", N.firingrate, ref))
    assert peaks >= 10 * T                              # near-peak elements did occur
    want, pos = np.array(N.history["firingrate"]), np.asarray(Ag.pos)
    Ag, N = world()
    plan = Ag.make_step_plan(capacity=T)
    for _ in range(T):
        plan.step()
    assert np.array_equal(np.asarray(Ag.pos), pos) and np.array_equal(np.array(N.history["firingrate"]), want)
    Ag, N = world()
    Ag.simulate(T)
    assert np.array_equal(np.asarray(Ag.pos), pos) and np.array_equal(np.array(N.history["firingrate"]), want)
    return worst


@pytest.mark.parametrize("width", vc.WIDTHS)
def test_narrow_head_direction_cells_stepping_paths(riab, width):
    _stepping_paths(riab, riab.HeadDirectionCells, {"n": vc.HD_N, "angular_spread_degrees": width},
                    lambda Ag, N: orc.head_direction_cells(f32(Ag.head_direction), vc.HD_N, width))


def test_narrow_velocity_cells_stepping_paths(riab):
    _stepping_paths(riab, riab.VelocityCells, {"n": vc.HD_N, "angular_spread_degrees": 3.0},
                    lambda Ag, N: orc.velocity_cells(f32(Ag.velocity), vc.HD_N, N.one_sigma_speed, 3.0))


# ----------------------------------------------------------------------------- B. object counts
@pytest.mark.parametrize("M", vc.OBJECT_COUNTS)
def test_object_counts(riab, M):
    """Every cell count and both frames at 257 positions, every position count at 9 cells, 12 occluding walls."""
    full = vc.many_objects(M)
    Ag = riab.Agent(make_env(riab, full))
    shapes = [(n, 257) for n in vc.CELL_COUNTS] + [(9, P) for P in vc.POSITION_COUNTS if P != 257]
    for n, P in shapes:
        c = vc.many_objects(M, n=n, P=P)
        for ego in (False, True):
            O = make_ovc(riab, Ag, c, ego, True)
            terms = vc.ovc_terms(c, True, ego)
            check(f"ovc M={M} n={n} P={P} {'ego' if ego else 'allo'}", ovc_state(O, c, ego), terms.sum(axis=1).T,
                  extra=vc.sum_allowance(terms))


def test_object_counts_spikes_and_simulate(riab):
    """86 objects (the first count that needs the raised LDS limit): update() with Poisson spikes against the host Philox,
    then Agent.simulate(5), whose rate kernels are launched from the native run's own stream."""
    M, B, dt, seed = 86, 65, 0.05, 1234
    c = vc.many_objects(M, n=9, P=B)
    np.random.seed(3)
    Ag = riab.Agent(make_env(riab, c), {"n_agents": B, "dt": dt, "seed": seed})
    O = make_ovc(riab, Ag, c, True, True, max_fr=30.0)
    Ag.update()
    Ag.pos, Ag.head_direction = c["pos"], c["hd"]
    O.update()
    torch.cuda.synchronize()
    terms = vc.ovc_terms(c, True, True) * 30.0
    check("ovc M=86 update() with spikes", O.firingrate, terms.sum(axis=1).T, scale=30.0, extra=vc.sum_allowance(terms))
    fr, sp = O.get_history_tensors()
    u = orc.spike_uniforms(seed, 1, O.pop_id, 9, (B + 3) // 4 * 4)[:, :B]
    got = sp[-1][:, :B].cpu().numpy().astype(bool)
    assert np.array_equal(got, orc.spikes_f32(fr[-1][:, :B].cpu().numpy(), u, dt)) and got.sum() > 0
    # simulate(): the agents move on from where they were put
    np.random.seed(4)
    Ag2 = riab.Agent(make_env(riab, c), {"n_agents": 70, "dt": 0.02, "seed": 7})
    O2 = make_ovc(riab, Ag2, c, False, True)
    Ag2.simulate(5)
    torch.cuda.synchronize()
    assert Ag2.diagnostics["pipeline_timeouts"] == 0
    row = Ag2.get_history_tensor()[-1].cpu().numpy()
    c2 = dict(c, pos=row[0:2, :70].T.astype(np.float64))
    assert vc.occlusion_margins(c2)[0].min() > 1e-9       # (no line of sight of the run's own positions is a tie)
    terms = vc.ovc_terms(c2, True, False)
    check("ovc M=86 simulate(5)", O2.firingrate, terms.sum(axis=1).T, extra=vc.sum_allowance(terms))


def _too_big(riab, excinfo):
    L = riab._lib
    msg = str(excinfo.value)
    return f"code {L.ETOOBIG}:" in msg or L.strerror(L.ETOOBIG) in msg


@pytest.mark.parametrize("M", vc.REFUSED_COUNTS)
def test_object_counts_beyond_the_lds_are_refused(riab, M):
    """More objects than a workgroup's LDS holds: RIAB_ETOOBIG from get_state, update(), simulate() and a step plan,
    never a raw HIP error; a smaller population computes correctly right after on the same stream."""
    L = riab._lib
    c = vc.many_objects(M, n=3, P=65)
    np.random.seed(5)
    Ag = riab.Agent(make_env(riab, c), {"n_agents": 65, "dt": 0.05})
    O = make_ovc(riab, Ag, c, False, True)
    small = vc.many_objects(5, n=3, P=65)
    Ag5 = riab.Agent(make_env(riab, small), {"n_agents": 65})
    O5 = make_ovc(riab, Ag5, small, False, True)

    def small_is_right(what):
        check(f"ovc M=5 after the refusal of M={M} ({what})", ovc_state(O5, small, False), vc.ovc_reference(small, True, False))

    with pytest.raises(L.RiabError) as e:
        ovc_state(O, c, False)
    assert _too_big(riab, e), str(e.value)
    small_is_right("get_state")
    Ag.update()
    with pytest.raises(L.RiabError) as e:
        O.update()
    assert _too_big(riab, e), str(e.value)
    small_is_right("update")
    with pytest.raises(L.RiabError) as e:
        Ag.make_step_plan()
    assert _too_big(riab, e), str(e.value)
    with pytest.raises(L.RiabError) as e:
        Ag.simulate(3)
    assert _too_big(riab, e), str(e.value)
    small_is_right("simulate")
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- C. periodic rooms
def test_periodic_room(riab):
    c = vc.periodic_case()
    oenv = vc.periodic_env()
    room = dict(boundary_conditions="periodic", **vc.PERIODIC)
    env = make_env(riab, c, **room)
    Ag = riab.Agent(env)
    # the wrapped vectors themselves (float64 on the device): pairs more than `scale` apart along x keep the reference's sign
    far = np.abs(c["pos"][:, None, 0] - c["objects"][None, :, 0]) > vc.PERIODIC["scale"]
    assert far.sum() >= 20
    np.testing.assert_allclose(env.get_vectors_between___accounting_for_environment(c["pos"], c["objects"]),
                               orc.env_vectors_between(oenv, c["pos"], c["objects"]), rtol=0, atol=1e-15)
    for ego in (False, True):
        O = make_ovc(riab, Ag, c, ego, False)
        check(f"ovc periodic {'ego' if ego else 'allo'}", ovc_state(O, c, ego), vc.ovc_reference(c, False, ego, env=oenv))
    with pytest.raises(AssertionError, match="line of sight"):       # as the reference refuses it (Environment.py:711-713)
        ovc_state(make_ovc(riab, Ag, c, False, True), c, False)
    A, B = _two_agents(riab, riab.Environment(dict(room)), c)
    N = tune(riab.AgentVectorCells(A, B, {"n": len(c["mu_d"]), "reference_frame": "egocentric", "walls_occlude": False}), c)
    N.update()
    check("avc periodic", N.firingrate, vc.avc_reference(c, walls_occlude=False, env=oenv))
    with pytest.raises(AssertionError, match="line of sight"):
        tune(riab.AgentVectorCells(A, B, {"n": len(c["mu_d"])}), c).update()


# ----------------------------------------------------------------------------- D. changing objects, degenerate geometry
def _live_world(riab, c, B=70):
    np.random.seed(6)
    Ag = riab.Agent(make_env(riab, c), {"n_agents": B, "dt": 0.05, "seed": 21})
    return Ag, make_ovc(riab, Ag, c, False, True)


def _reference_at_agents(Ag, c, objects, types, B=70):
    row = Ag.get_history_tensor()[-1].cpu().numpy()
    return vc.ovc_reference(dict(c, pos=row[0:2, :B].T.astype(np.float64), objects=objects, object_types=types), True, False)


def test_add_object_under_a_live_population(riab):
    """env.add_object after the population exists: update() and simulate() (the second call through the repeat path) see
    the new object at once; a recorded step plan is closed and refuses its next step."""
    c = vc.narrow_ovc(10.0, False)
    new = f32([0.42, 0.61])
    objects, types = np.vstack((c["objects"], new[None])), np.append(c["object_types"], 0)
    # between two update() calls
    Ag, O = _live_world(riab, c)
    Ag.update()
    O.update()
    check("add_object: update() before", O.firingrate, _reference_at_agents(Ag, c, c["objects"], c["object_types"]))
    Ag.Environment.add_object(new, type=0)
    Ag.update()
    O.update()
    after = _reference_at_agents(Ag, c, objects, types)
    assert (np.abs(after - _reference_at_agents(Ag, c, c["objects"], c["object_types"])) > 1e-4).any()   # it matters
    check("add_object: update() after", O.firingrate, after)
    # between two simulate() calls
    Ag, O = _live_world(riab, c)
    Ag.simulate(4)
    Ag.simulate(4)                                      # (the repeat path is warm)
    check("add_object: simulate() before", O.firingrate, _reference_at_agents(Ag, c, c["objects"], c["object_types"]))
    Ag.Environment.add_object(new, type=0)
    Ag.simulate(4)
    torch.cuda.synchronize()
    check("add_object: simulate() after", O.firingrate, _reference_at_agents(Ag, c, objects, types))
    # after make_step_plan()
    Ag, O = _live_world(riab, c)
    plan = Ag.make_step_plan(capacity=8)
    plan.step()
    check("add_object: plan before", O.firingrate, _reference_at_agents(Ag, c, c["objects"], c["object_types"]))
    Ag.Environment.add_object(new, type=0)
    with pytest.raises(RuntimeError, match="closed"):
        plan.step()
    plan = Ag.make_step_plan(capacity=8)                # a new plan records the new object list
    plan.step()
    check("add_object: new plan after", O.firingrate, _reference_at_agents(Ag, c, objects, types))


def test_degenerate_geometry(riab):
    c = vc.degenerate_case()
    Ag = riab.Agent(make_env(riab, c))
    for ego in (False, True):
        O = make_ovc(riab, Ag, c, ego, False)
        got = ovc_state(O, c, ego)
        assert np.isfinite(got).all()
        check(f"ovc degenerate {'ego' if ego else 'allo'}", got, vc.ovc_reference(c, False, ego))
    H = riab.HeadDirectionCells(Ag, {"n": 12, "angular_spread_degrees": 10.0})
    check("hdc head direction (0, 0)", H.get_state(evaluate_at=None, pos=c["pos"], head_direction=c["hd"]),
          orc.head_direction_cells(c["hd"], 12, 10.0))
