"""Guard bands around every kernel's output rows at ragged shapes (tests/guard_arena.py; tests/test_guard_arena_cpu.py shows
that the checker finds what is planted).

The value tests pin WHAT the kernels write; these pin WHERE.  Every output is a view in the middle of a canary-filled
allocation, every case runs once with a NaN canary and once with a finite one, and `check` asserts: both guards untouched,
every interior element written, the same interior bits whatever the memory held before.  The interior is compared with the
float64 oracle in the same call, with the tolerance the population already has in tests/test_gpu_parity.py (imported, none
new).  Shapes are the smallest that are ragged against each kernel's tiling; with T = 1 every store past the last cell lands
in the back guard, with T = 3 the last row's does.

(a) every population through its own `_launch`;  (b) the BVC ray stage's `ray_out`;  (c) `riab_spikes` and
`riab_neuron_noise` alone;  (d) the motion kernel;  (e) the streamed and planned forms, whose buffers the package owns: the
free tail of the history chunk is the guard;  (f) one positive control: a legitimate extra row that lands in the back guard
must be reported, and at the right place."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import riab_oracle as orc
from tests import bvc_ray_cases as bc
from tests import guard_arena as ga
from tests import nn_modules, nn_oracle
from tests import plane_wave_oracle as pwo
from tests import theta_oracle as tho
from tests.test_gpu_noise import assert_noise, f32
from tests.test_gpu_parity import assert_discrete_mismatches_are_ties, assert_rates
from tests.test_gpu_plane_wave import _check as assert_plane_wave

pytestmark = pytest.mark.gpu

SEED, STEP0, ID0, DT = 0x1234567800000321, 5, 4096, 0.05
MIN_FR, MAX_FR = 0.5, 8.0
RANGE = MAX_FR - MIN_FR
WALL = [[[0.5, 0.1], [0.5, 0.6]]]                # one interior wall: line of sight, geodesic, the BVC's full wall test
OBJECTS = [([0.3, 0.3], 0), ([0.7, 0.6], 1), ([0.25, 0.8], 0)]


@pytest.fixture(scope="module")
def riab():
    assert torch.cuda.is_available(), "these tests need the GPU"
    import ratinabox_amd
    return ratinabox_amd


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


_ROWS = {}


def rows_of(T, B):
    """positions (T, 2, B) inside the room, unit head directions and velocities (T, 2, B): float32, drawn once per shape"""
    if (T, B) not in _ROWS:
        rs = np.random.RandomState(1000 * T + B)
        pos = rs.uniform(0.02, 0.98, (T, 2, B)).astype(np.float32)
        ang = rs.uniform(0, 2 * np.pi, (T, B))
        hd = np.stack((np.cos(ang), np.sin(ang)), 1).astype(np.float32)
        vel = rs.normal(0, 0.15, (T, 2, B)).astype(np.float32)
        _ROWS[(T, B)] = dict(pos=pos, hd=hd, vel=vel)
    return _ROWS[(T, B)]


def P(rows, t, key="pos"):
    """(B, 2) float64 of time row t"""
    return rows[key][t].T.astype(np.float64)


def per_row(T, reference, compare):
    """verify(fr): compare(fr[t], reference(t), t) for every time row; a row's reference is computed once per case"""
    refs = {}

    def verify(fr):
        for t in range(T):
            if t not in refs:
                refs[t] = reference(t)
            compare(fr[t], refs[t], t)
    return verify


def world(riab, B, env_params=None, objects=(), **agent):
    env = riab.Environment(dict(env_params or {}))
    for o, ty in objects:
        env.add_object(o, type=ty)
    return env, riab.Agent(env, dict({"n_agents": B, "dt": DT, "seed": SEED, "agent_id0": ID0}, **agent))


def guarded(N, T, B, rows, verify, spike_modes=("none", "philox", "explicit"), direction="hd", launch=None):
    """N._launch (or `launch`, same arguments) on arena views, for every spike mode and both canaries: guards, unwritten
    elements and canary dependence by `check`; the rates by `verify(fr (T, n, B))`; the spike bytes against the rule on the
    call's own rates with the host-regenerated Philox uniforms, or the explicit ones it was handed."""
    n, Ag = int(N.n), N.Agent
    assert Ag._Bp == B
    px, py = dev(rows["pos"][:, 0]), dev(rows["pos"][:, 1])
    hx, hy = dev(rows[direction][:, 0]), dev(rows[direction][:, 1])
    u = np.random.RandomState(7 * T + B + n).uniform(0, 1, (T, n, B)).astype(np.float32)
    n_spikes = 0
    for spk in spike_modes:
        first = {}
        for canary in ga.CANARIES:
            arena = ga.GuardArena(canary)
            rates = arena.view((T, n, B), torch.float32, "cuda")
            spikes = arena.view((T, n, B), torch.uint8, "cuda") if spk != "none" else None
            u_t = dev(u) if spk == "explicit" else None
            (launch or N._launch)(px, py, hx, hy, B, T, B, rates, spikes, u_t, DT, STEP0)
            torch.cuda.synchronize()
            first.setdefault("fr", arena.check(rates, other=first.get("fr")))
            if spikes is not None:
                first.setdefault("sp", arena.check(spikes, other=first.get("sp")))
        fr = first["fr"]
        verify(fr)
        if spk != "none":
            sp = first["sp"]
            assert (sp <= 1).all()
            for t in range(T):
                uu = u[t] if spk == "explicit" else orc.spike_uniforms(SEED, STEP0 + t, N.pop_id, n, B, agent_id0=ID0)
                assert np.array_equal(sp[t].astype(bool), orc.spikes_f32(fr[t], uu, DT)), (spk, t)
            n_spikes += int(sp.sum())
    if len(spike_modes) > 1 and T * n * B >= 1000 and float(np.mean(first["fr"])) > 1.0:
        assert n_spikes > 0      # (dt * rate > 0.05 per element on average: thousands of draws)


# ---------------------------------------------------------------------------------------------------------------------
# (a) populations.  A variant: name -> make(riab, B, n, T, rows) -> (population, verify, keyword arguments of `guarded`)
# ---------------------------------------------------------------------------------------------------------------------
def _place(desc, geom):
    def make(riab, B, n, T, rows):
        periodic = geom == "periodic"
        g = "euclidean" if periodic else geom
        walls = WALL if g in ("line_of_sight", "geodesic") else []
        bc_ = "periodic" if periodic else "solid"
        env, Ag = world(riab, B, {"walls": walls, "boundary_conditions": bc_})
        N = riab.PlaceCells(Ag, {"n": n, "description": desc, "widths": 0.2, "wall_geometry": g, "min_fr": MIN_FR, "max_fr": MAX_FR})
        assert N.wall_geometry == g
        oenv = orc.EnvSpec(walls=walls, boundary_conditions=bc_)
        c = np.asarray(N.place_cell_centres)

        def reference(t):
            return orc.place_cells(oenv, P(rows, t), c, 0.2, description=desc, wall_geometry=g, min_fr=MIN_FR, max_fr=MAX_FR,
                                   widths_scalar=0.2)

        def compare(fr, ref, t):
            if desc in ("one_hot", "top_hat"):
                assert_discrete_mismatches_are_ties(fr, ref, orc.env_distances(oenv, c, P(rows, t), g), desc, width=0.2)
            else:
                assert_rates(fr, ref, scale=RANGE, floor=0.0 if desc == "gaussian" else 1.0)
        return N, per_row(T, reference, compare), {}
    return make


def _grid(desc):
    def make(riab, B, n, T, rows):
        env, Ag = world(riab, B)
        N = riab.GridCells(Ag, {"n": n, "description": desc, "min_fr": MIN_FR, "max_fr": MAX_FR})

        def verify(fr):
            for t in range(T):
                ref = orc.grid_cells(P(rows, t), N.gridscales, N.phase_offsets, N.w, description=desc, min_fr=MIN_FR, max_fr=MAX_FR)
                assert_rates(fr[t], ref, scale=RANGE, floor=1.0)
        return N, verify, {}
    return make


def _hdc(riab, B, n, T, rows):
    env, Ag = world(riab, B)
    N = riab.HeadDirectionCells(Ag, {"n": n, "min_fr": MIN_FR, "max_fr": MAX_FR})

    def verify(fr):
        for t in range(T):
            assert_rates(fr[t], orc.head_direction_cells(P(rows, t, "hd"), n, 45.0, MIN_FR, MAX_FR))
    return N, verify, {}


def _velocity(riab, B, n, T, rows):
    """from float32 rows: the velocity is read where the other kernels read the head direction (vel_x == NULL)"""
    env, Ag = world(riab, B)
    N = riab.VelocityCells(Ag, {"n": n, "min_fr": MIN_FR, "max_fr": MAX_FR})

    def verify(fr):
        for t in range(T):
            assert_rates(fr[t], orc.velocity_cells(P(rows, t, "vel"), n, N.one_sigma_speed, 45.0, MIN_FR, MAX_FR))
    return N, verify, dict(direction="vel")


def _speed(riab, B, n, T, rows):
    env, Ag = world(riab, B)
    N = riab.SpeedCell(Ag, {"min_fr": MIN_FR, "max_fr": MAX_FR})

    def verify(fr):
        for t in range(T):
            assert_rates(fr[t], orc.speed_cell(P(rows, t, "vel"), N.one_sigma_speed, MIN_FR, MAX_FR))
    return N, verify, dict(direction="vel")


def _random_spatial(riab, B, n, T, rows):
    env, Ag = world(riab, B, {"walls": WALL})
    N = riab.RandomSpatialNeurons(Ag, {"n": n, "lengthscale": 0.1, "wall_geometry": "geodesic", "min_fr": MIN_FR, "max_fr": MAX_FR})
    oenv = orc.EnvSpec(walls=WALL)
    return N, per_row(T, lambda t: orc.random_spatial_neurons(oenv, P(rows, t), N.X, N.targets, 0.1, "geodesic"),
                      lambda fr, ref, t: assert_rates(fr, ref)), {}


def _plane_wave(riab, B, n, T, rows):
    from ratinabox_amd.contribs.PlaneWaveNeurons import PlaneWaveNeurons
    env, Ag = world(riab, B)
    N = PlaneWaveNeurons(Ag, {"n": n, "wavescale": 0.2, "min_fr": MIN_FR, "max_fr": MAX_FR})
    tab = N._call(None, None)["table"].cpu().numpy()

    def verify(fr):
        for t in range(T):
            assert_plane_wave(fr[t], pwo.rates(P(rows, t), N.phase_offsets, N.w, N.wavescales, MIN_FR, MAX_FR), tab, P(rows, t),
                              RANGE, f"guard bands n={n} B={B} t={t}")
    return N, verify, {}


def _theta(riab, B, n, T, rows):
    """T = 1 only (its ABI limit: one clock and the float64 velocity state per call).  The bound is the plain project
    criterion, assert_rates with floor 1 on the range, which docs/EXPERIMENTS.md "Theta phase precession" records the
    kernel inside of by a factor 5 (test_gpu_theta.py's own yardstick, the worst ratio of an fp32 NumPy run over hundreds
    of samples, is no bound for four of them)."""
    from ratinabox_amd.contribs.PhasePrecessingPlaceCells import PhasePrecessingPlaceCells
    assert T == 1
    env, Ag = world(riab, B)
    N = PhasePrecessingPlaceCells(Ag, {"n": n, "description": "gaussian", "widths": 0.25, "kappa": 2.0, "theta_freq": 10.0,
                                       "precess_fraction": 0.5, "min_fr": MIN_FR, "max_fr": MAX_FR, "wall_geometry": "euclidean"})
    vel = P(rows, 0, "vel")
    Ag.velocity, Ag.t = vel if B > 1 else vel[0], 0.437
    N._modulated = True            # (what update() and get_state("agent") set around their launch)

    def verify(fr):
        ref = tho.rates(P(rows, 0), vel, Ag.t, N.place_cell_centres, N.place_cell_widths, "gaussian", 10.0, 2.0, 0.5, MIN_FR, MAX_FR,
                        widths_scalar=0.25)
        assert_rates(fr[0], ref, scale=RANGE, floor=1.0)
    return N, verify, {}


GENERIC = {f"place-{d}-{g}": _place(d, g) for d in ("gaussian", "one_hot")
           for g in ("euclidean", "line_of_sight", "geodesic", "periodic")}
GENERIC.update({f"place-{d}-euclidean": _place(d, "euclidean") for d in ("gaussian_threshold", "diff_of_gaussians", "top_hat")})
GENERIC.update({"grid-rectified_cosines": _grid("rectified_cosines"), "grid-shifted_cosines": _grid("shifted_cosines"),
                "hdc": _hdc, "velocity": _velocity, "speed": _speed, "random_spatial": _random_spatial,
                "plane_wave": _plane_wave, "theta_place": _theta})
# generic / one_hot / random-spatial kernels: 256 quads per workgroup, 64-cell chunks; the wide kernel: qrow >= 256, 4 or 16
# cells per group, T = 1 with write-through stores
GENERIC_SHAPES = [(B, n, T) for B in (4, 260) for n in (1, 5, 65) for T in (1, 3)] + \
                 [(1028, n, T) for n in (5, 17) for T in (1, 3)]


def _generic_cases():
    for name in GENERIC:
        for B, n, T in GENERIC_SHAPES:
            if name == "theta_place" and T != 1:
                continue
            if name == "speed" and n != (1 if B != 1028 else 5):      # one cell, whatever is asked for: once per (B, T)
                continue
            yield pytest.param(name, B, n, T, id=f"{name}-B{B}-n{n}-T{T}")


@pytest.mark.parametrize("name,B,n,T", list(_generic_cases()))
def test_rate_kernels(riab, name, B, n, T):
    np.random.seed(100 * n + B)
    rows = rows_of(T, B)
    N, verify, kw = GENERIC[name](riab, B, n, T, rows)
    guarded(N, T, B, rows, verify, **kw)


# ---- BVC / OVC / AVC: 64-position tiles, 4-cell blocks ---------------------------------------------------------------
def _bvc(frame):
    def make(riab, B, n, T, rows):
        env, Ag = world(riab, B, {"walls": WALL})
        N = riab.BoundaryVectorCells(Ag, {"n": n, "reference_frame": frame, "min_fr": MIN_FR, "max_fr": MAX_FR})
        return N, _bvc_verify(env, N, T, rows, frame == "egocentric")
    return make


def _bvc_verify(env, N, T, rows, ego):
    def reference(t):
        kw = dict(head_direction=P(rows, t, "hd")) if ego else {}
        return orc.bvc(P(rows, t), env.walls, N.tuning_distances, N.tuning_angles, N.sigma_distances, N.sigma_angles,
                       min_fr=MIN_FR, max_fr=MAX_FR, **kw)
    return per_row(T, reference, lambda fr, ref, t: assert_rates(fr, ref, scale=RANGE, floor=1.0))


def _fov_bvc(riab, B, n, T, rows):
    env, Ag = world(riab, B, {"walls": WALL})
    N = riab.FieldOfViewBVCs(Ag, {"cell_arrangement": "uniform_manifold", "distance_range": [0.05, 0.3], "angle_range": [0, 120],
                                  "spatial_resolution": 0.05, "min_fr": MIN_FR, "max_fr": MAX_FR})
    return N, _bvc_verify(env, N, T, rows, True)


def _ovc(occlude):
    def make(riab, B, n, T, rows):
        env, Ag = world(riab, B, {"walls": WALL}, OBJECTS)
        N = riab.ObjectVectorCells(Ag, {"n": n, "walls_occlude": occlude, "min_fr": MIN_FR, "max_fr": MAX_FR})
        oenv = orc.EnvSpec(walls=WALL)

        def reference(t):
            return orc.object_vector_cells(oenv, P(rows, t), env.objects["objects"], env.objects["object_types"],
                                           N.tuning_distances, N.tuning_angles, N.sigma_distances, N.sigma_angles, N.tuning_types,
                                           walls_occlude=occlude, min_fr=MIN_FR, max_fr=MAX_FR)
        return N, per_row(T, reference, lambda fr, ref, t: assert_rates(fr, ref, scale=RANGE, floor=1.0))
    return make


def _avc(riab, B, n, T, rows):
    env, Ag = world(riab, B, {"walls": WALL})
    Other = riab.Agent(env, {"n_agents": B, "dt": DT, "seed": SEED + 1, "agent_id0": ID0})
    other = np.random.RandomState(B).uniform(0.05, 0.95, (B, 2)).astype(np.float32).astype(np.float64)
    Other.pos = other
    N = riab.AgentVectorCells(Ag, Other, {"n": n, "min_fr": MIN_FR, "max_fr": MAX_FR})
    oenv = orc.EnvSpec(walls=WALL)

    def reference(t):
        return orc.agent_vector_cells(oenv, P(rows, t), other, N.tuning_distances, N.tuning_angles, N.sigma_distances,
                                      N.sigma_angles, walls_occlude=True, min_fr=MIN_FR, max_fr=MAX_FR)
    return N, per_row(T, reference, lambda fr, ref, t: assert_rates(fr, ref, scale=RANGE, floor=1.0))


VECTOR = {"bvc-allocentric": _bvc("allocentric"), "bvc-egocentric": _bvc("egocentric"), "fov_bvc": _fov_bvc,
          "ovc-occluded": _ovc(True), "ovc-open": _ovc(False), "avc": _avc}


def _vector_cases():
    for name in VECTOR:
        for B in (4, 68):
            for n in (1, 5):
                for T in (1, 3):
                    if name == "fov_bvc" and n != 5:       # (the manifold sets its own cell count)
                        continue
                    yield pytest.param(name, B, n, T, id=f"{name}-B{B}-n{n}-T{T}")


@pytest.mark.parametrize("name,B,n,T", list(_vector_cases()))
def test_vector_cell_kernels(riab, name, B, n, T):
    np.random.seed(100 * n + B)
    rows = rows_of(T, B)
    N, verify = VECTOR[name](riab, B, n, T, rows)
    guarded(N, T, B, rows, verify, spike_modes=("none", "philox"))


# ---- FeedForwardLayer: ff_kernel, 128 positions x 32 outputs ---------------------------------------------------------
N_IN = (17, 3)


def _carriers(riab, Ag):
    """two populations whose `_rates` rows carry the test's own inputs (their kernels are not run)"""
    return [riab.PlaceCells(Ag, {"n": N_IN[0], "name": "in0"}), riab.GridCells(Ag, {"n": N_IN[1], "name": "in1"})]


def _inputs(T, B):
    rs = np.random.RandomState(31 * T + B)
    return [rs.uniform(0, 1, (T, k, B)).astype(np.float32) for k in N_IN]


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("B", [4, 132])
def test_feedforward_layer(riab, B, n, T):
    """rates AND `out_prime` in arenas.  T = 1 through FeedForwardLayer._launch (the inputs' last rates, `_rates_prime`);
    T = 3 through `_gemm` and `_spike_pass`, as the streamed form calls them.  Bound: test_randomised_feedforward_shapes_vs_oracle's
    (inputs in [0, 1]); the relu derivative is 0 or the gain: a mismatch must be a tie of `x > threshold` within that bound."""
    np.random.seed(100 * n + B)
    rs = np.random.RandomState(6000 + n + B)
    env, Ag = world(riab, B)
    layers = _carriers(riab, Ag)
    spec = {"activation": "relu", "gain": 1.3, "threshold": -0.1}
    bias = rs.normal(0, 0.3, n)
    F = riab.FeedForwardLayer(Ag, {"n": n, "input_layers": layers, "activation_function": spec, "biases": bias.copy()})
    ws = []
    for L_ in layers:
        w = rs.normal(0, 1 / np.sqrt(L_.n), (n, L_.n))
        F.inputs[L_.name]["w"] = w.copy()
        ws.append(w.astype(np.float32).astype(np.float64))
    xs = _inputs(T, B)
    xs_dev = [dev(x) for x in xs]
    b32 = bias.astype(np.float32).astype(np.float64)
    cond = sum(np.abs(w).sum(1) for w in ws) + np.abs(bias)
    L = riab._lib
    for spk in ("none", "philox"):
        first = {}
        for canary in ga.CANARIES:
            arena = ga.GuardArena(canary)
            rates, prime = (arena.view((T, n, B), torch.float32, "cuda") for _ in range(2))
            spikes = arena.view((T, n, B), torch.uint8, "cuda") if spk != "none" else None
            if T == 1:
                for L_, x in zip(layers, xs_dev):
                    L_._rates = x[0]
                F._rates_prime = prime[0]
                F._launch(None, None, None, None, B, 1, B, rates, spikes, None, DT, STEP0)
            else:
                F._gemm(xs_dev, T, B, rates, prime, L.current_stream())
                if spikes is not None:
                    F._spike_pass(rates, spikes, None, DT, STEP0)
            torch.cuda.synchronize()
            first.setdefault("fr", arena.check(rates, other=first.get("fr")))
            first.setdefault("prime", arena.check(prime, other=first.get("prime")))
            if spikes is not None:
                first.setdefault("sp", arena.check(spikes, other=first.get("sp")))
        for t in range(T):
            ins = [x[t].astype(np.float64) for x in xs]
            ref, dref = orc.feedforward(ins, ws, b32, spec)
            tol = 2e-6 * cond[:, None] * spec["gain"] + 1e-6 * np.abs(ref)
            err = np.abs(first["fr"][t] - ref)
            assert (err <= tol).all(), (t, err.max())
            pre = sum(w @ x for w, x in zip(ws, ins)) + b32[:, None]
            off = first["prime"][t] != dref.astype(np.float32)
            assert (np.abs(pre - spec["threshold"])[off] <= 2e-6 * np.broadcast_to(cond[:, None], pre.shape)[off]).all()
            if spk != "none":
                uu = orc.spike_uniforms(SEED, STEP0 + t, F.pop_id, n, B, agent_id0=ID0)
                assert np.array_equal(first["sp"][t].astype(bool), orc.spikes_f32(first["fr"][t], uu, DT))


# ---- NeuralNetworkNeurons, fused engine: mlp_kernel, 32 positions per wave, 32-row output tiles ------------------------
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("B", [4, 36, 132])
def test_neural_network_neurons(riab, B, n, T):
    """T = 1 through NeuralNetworkNeurons._launch, T = 3 through `_forward` and `_spike_pass` (the streamed form's calls);
    the bound is the one tests/nn_oracle.forward returns."""
    from ratinabox_amd.contribs.NeuralNetworkNeurons import NeuralNetworkNeurons
    np.random.seed(100 * n + B)
    torch.manual_seed(100 * n + B)
    env, Ag = world(riab, B)
    layers = _carriers(riab, Ag)
    module = nn.Sequential(nn.Linear(sum(N_IN), 20), nn.ReLU(), nn.Linear(20, 33), nn.Tanh(), nn.Linear(33, n))
    N = NeuralNetworkNeurons(Ag, {"input_layers": layers, "NeuralNetworkModule": module})
    assert N.engine == "fused" and int(N.n) == n
    lins = [m for m in module.modules() if type(m) is nn.Linear]
    spec = nn_modules.module_layers(list(zip(lins, ["relu", "tanh", "linear"])))
    xs = _inputs(T, B)
    xs_dev = [dev(x) for x in xs]
    want = [nn_oracle.forward(spec, np.concatenate([x[t] for x in xs]).astype(np.float64)) for t in range(T)]

    def launch(px, py, hx, hy, pos_ld, T_, B_, rates, spikes, u_in, dt, step0):
        if T == 1:
            for L_, x in zip(layers, xs_dev):
                L_._rates = x[0]
            return N._launch(px, py, hx, hy, pos_ld, T_, B_, rates, spikes, u_in, dt, step0)
        N._forward(xs_dev, T, B, rates, riab._lib.current_stream())
        if spikes is not None:
            N._spike_pass(rates, spikes, u_in, dt, step0)

    def verify(fr):
        for t in range(T):
            ref, tol = want[t]
            err = np.abs(fr[t] - ref)
            assert (err <= tol).all(), (t, err.max(), (err / tol).max())
    guarded(N, T, B, rows_of(T, B), verify, spike_modes=("none", "philox"), launch=launch)


# ---------------------------------------------------------------------------------------------------------------------
# (b) the BVC ray stage: ray_out [T][K][B], K = 51 (dtheta = 7: ragged against 4, odd, a pad row)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("B", [4, 68])
def test_bvc_ray_out(riab, B, T):
    """through riab_boundary_vector_cells_windowed as tests/test_gpu_bvc_rays.py calls it, `ray_out` and the rates in
    arenas; the rays against oracle.bvc_ray_distances under that file's bound (bvc_ray_cases.ray_tolerance), none left out
    (positions strictly inside the maze)."""
    import ctypes as C
    L = riab._lib
    r, (angles, dirs) = bc.room("maze"), bc.table("K51")
    K, n, pos_ld = len(dirs), 5, B + 4
    pos = r["inside"](np.random.RandomState(50 + T + B), T * B).reshape(T, B, 2)
    ref, first, l_a, l_b = bc.oracle_rays(pos.reshape(-1, 2), r["walls"], dirs)
    assert not bc.exclusions(ref, first, l_a, l_b).any()
    bound = bc.ray_tolerance(pos.reshape(-1, 2), r["walls"], dirs, ref, first)
    mu_d, sg_d, mu_t, sg_t = bc.stage_b_cells(n)
    tabs = bc.bvc_tables(r["walls"], angles, dirs, mu_d, sg_d, mu_t, sg_t, False)
    d = {k: dev(v, np.float64 if k in ("test_dirs", "ray_rden") else np.float32) for k, v in tabs.items() if k != "K"}
    walls = dev(np.asarray(r["walls"]).reshape(-1, 4), np.float64)
    env = L.RiabEnv()
    for i in range(4):
        env.extent[i] = float(r["extent"][i])
    env.scale, env.periodic, env.n_walls, env.walls = 1.0, 0, int(len(walls)), walls.data_ptr()
    env.polygon, env.n_boundary, env.hole_mask = int(r["polygon"]), int(r["n_boundary"]), 0

    def padded(a):
        t = torch.full((T, pos_ld), 1e30, dtype=torch.float32)
        t[:, :B] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        return t.cuda()
    px, py = padded(pos[..., 0]), padded(pos[..., 1])
    got = {}
    for canary in ga.CANARIES:
        arena = ga.GuardArena(canary)
        rays = arena.view((T, K, B), torch.float32, "cuda")
        rates = arena.view((T, n, B), torch.float32, "cuda")
        io = L.RiabRateIO()
        io.pos_x, io.pos_y, io.pos_ld, io.T, io.B = px.data_ptr(), py.data_ptr(), pos_ld, T, B
        io.rates, io.dt, io.min_fr, io.max_fr = rates.data_ptr(), DT, 0.0, 1.0
        rc = L.lib.riab_boundary_vector_cells_windowed(env, io, L.ptr(d["test_dirs"]), L.ptr(d["ray_rden"]), K, L.ptr(d["cells"]),
                                                       L.ptr(d["vm"]), L.ptr(d["inv_norm"]), n, 0, C.c_void_p(rays.data_ptr()),
                                                       None, None, L.current_stream())
        assert rc == 0, L.strerror(rc)
        torch.cuda.synchronize()
        got.setdefault("rays", arena.check(rays, other=got.get("rays")))
        got.setdefault("rates", arena.check(rates, other=got.get("rates")))
    x = got["rays"].transpose(0, 2, 1).reshape(T * B, K).astype(np.float64)        # ray_out is indexed (t K + k) B + b
    err = np.abs(x - ref.astype(np.float32).astype(np.float64))
    assert (err <= bound).all(), (err / bound).max()
    assert np.isfinite(got["rates"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# (c) riab_spikes and riab_neuron_noise alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("explicit", [False, True], ids=["philox", "explicit"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("B", [4, 260])
def test_spikes_alone(riab, B, T, explicit):
    """the rates are an INPUT here: their arena shows that the kernel leaves them, and what lies around them, alone"""
    L, n = riab._lib, 5
    rs = np.random.RandomState(B + T)
    fr = rs.uniform(0.0, 12.0, (T, n, B)).astype(np.float32)
    u = rs.uniform(0, 1, (T, n, B)).astype(np.float32)
    u_t = dev(u) if explicit else None
    first = None
    for canary in ga.CANARIES:
        arena = ga.GuardArena(canary)
        rates = arena.view((T, n, B), torch.float32, "cuda")
        rates.copy_(dev(fr))
        spikes = arena.view((T, n, B), torch.uint8, "cuda")
        io = L.RiabRateIO()
        io.pos_ld, io.T, io.B = B, T, B
        io.rates, io.spikes, io.u_in = rates.data_ptr(), spikes.data_ptr(), (u_t.data_ptr() if explicit else None)
        io.dt, io.min_fr, io.max_fr = DT, 0.0, 12.0
        io.seed, io.step0, io.agent_id0, io.pop_id = SEED, STEP0, ID0, 3
        rc = L.lib.riab_spikes(io, n, L.current_stream())
        assert rc == 0, L.strerror(rc)
        torch.cuda.synchronize()
        arena.check(rates, other=fr)                    # bit for bit what went in
        first = arena.check(spikes, other=first)
    assert (first <= 1).all() and first.sum() > 0
    for t in range(T):
        uu = u[t] if explicit else orc.spike_uniforms(SEED, STEP0 + t, 3, n, B, agent_id0=ID0)
        assert np.array_equal(first[t].astype(bool), orc.spikes_f32(fr[t], uu, DT)), t


@pytest.mark.parametrize("explicit", [False, True], ids=["philox", "explicit"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("B", [4, 260])
def test_neuron_noise_alone(riab, B, T, explicit):
    """the noise state [n][B] and the rates [T][n][B] are read AND written: both start from values of the test's own (so no
    element can show as unwritten by its bits; one that the kernel skipped is off by a whole noise term, a thousand times
    the bound).  Against the oracle's OU path from x0 on noise_normals (or the explicit normals), tolerances of
    tests/test_gpu_noise.py."""
    L, n, pop_id = riab._lib, 5, 3
    noise_std, tau = 0.4, 0.25
    theta_dt, sigma_dt = f32(DT / tau), f32(np.sqrt(2 * noise_std ** 2 / (tau * DT)) * DT)
    rs = np.random.RandomState(3 * B + T)
    x0 = rs.normal(0, noise_std, (n, B)).astype(np.float32)
    base = rs.uniform(1.0, 9.0, (T, n, B)).astype(np.float32)
    z = rs.normal(0, 1, (T, n, B)).astype(np.float32)
    z_t = dev(z) if explicit else None
    got = {}
    for canary in ga.CANARIES:
        arena = ga.GuardArena(canary)
        noise = arena.view((n, B), torch.float32, "cuda")
        rates = arena.view((T, n, B), torch.float32, "cuda")
        noise.copy_(dev(x0))
        rates.copy_(dev(base))
        rc = L.lib.riab_neuron_noise(L.ptr(noise), L.ptr(rates), L.ptr(z_t), n, B, T, theta_dt, sigma_dt, SEED, STEP0, pop_id, ID0,
                                     L.current_stream())
        assert rc == 0, L.strerror(rc)
        torch.cuda.synchronize()
        got.setdefault("noise", arena.check(noise, other=got.get("noise")))
        got.setdefault("rates", arena.check(rates, other=got.get("rates")))
    zz = z.astype(np.float64) if explicit else np.stack([orc.noise_normals(SEED, STEP0 + t, pop_id, n, B, agent_id0=ID0)
                                                         for t in range(T)])
    x = orc.ou_noise_path(zz, theta_dt, sigma_dt, x0=x0.astype(np.float64))
    assert_noise(got["rates"], base.astype(np.float64) + x, noise_std, rates=base, what=f"B={B} T={T}")
    assert_noise(got["noise"], x[-1], noise_std, what="state")


# ---------------------------------------------------------------------------------------------------------------------
# (d) motion: torch.ops.riab.agent_step_ with the state [12][B] and the history rows [steps][8][B] in arenas
# ---------------------------------------------------------------------------------------------------------------------
L_ROOM = [[0, 0], [1, 0], [1, 0.5], [0.5, 0.5], [0.5, 1], [0, 1]]
HOLE = [[0.2, 0.15], [0.4, 0.15], [0.4, 0.35], [0.2, 0.35]]
_STATE_ROWS = dict(pos=(0, 2), velocity=(2, 4), rotational_velocity=(4, 5), measured_velocity=(5, 7),
                   measured_rotational_velocity=(7, 8), head_direction=(8, 10), distance_travelled=(10, 11),
                   distance_to_closest_wall=(11, 12))


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("B", [4, 68])
@pytest.mark.parametrize("room", ["wall", "polygon_hole"])
def test_motion_kernel(riab, room, B, steps):
    """One interior wall (the box fast path and a wall to bounce off), then an L-shaped boundary with a hole in which every
    third agent starts: both wall paths store, and so does the resample branch (explicit replacement positions).  State and
    history rows against the oracle's step on the same explicit normals, tolerances of test_motion_single_steps_vs_reference
    (float64 state 1e-9; the fp32 arctangent behind the measured rotational velocity 2e-6) and of the rollout tests for the
    fp32 history rows."""
    from ratinabox_amd import ops
    np.random.seed(7 + B)
    if room == "wall":
        envp, oenv = {"walls": WALL}, orc.EnvSpec(walls=WALL)
    else:
        envp, oenv = {"boundary": L_ROOM, "holes": [HOLE]}, orc.EnvSpec(boundary=L_ROOM, holes=[HOLE])
    env, Ag = world(riab, B, envp, speed_mean=0.3 if room == "wall" else 0.08)
    rs = np.random.RandomState(B + steps)
    pos = np.array(Ag.pos, dtype=np.float64).reshape(B, 2)
    in_hole = np.zeros(B, dtype=bool)
    if room == "polygon_hole":
        in_hole[::3] = True
        pos[in_hole] = np.mean(HOLE, axis=0) + 0.01 * (rs.rand(int(in_hole.sum()), 2) - 0.5)
        Ag.pos = pos
        assert not orc.env_is_inside(oenv, pos[in_hole]).any() and orc.env_is_inside(oenv, pos[~in_hole]).all()
    st = {k: np.array(getattr(Ag, k), dtype=np.float64).reshape(B, -1) for k in
          ("pos", "velocity", "rotational_velocity", "measured_velocity", "head_direction", "distance_travelled")}
    for k in ("rotational_velocity", "distance_travelled"):
        st[k] = st[k][:, 0]
    st.update(measured_rotational_velocity=np.zeros(B), distance_to_closest_wall=np.full(B, np.inf))
    state0 = Ag.state_tensor.clone()
    assert tuple(state0.shape) == (12, B)
    z = rs.normal(0, 1, (steps, 2, B))
    resample = np.stack((rs.uniform(0.05, 0.45, (steps, B)), rs.uniform(0.55, 0.95, (steps, B))), axis=1)   # in the L's arm
    w_op, e_op, periodic = env.op_env_args(Ag._device)
    m = ops.motion_list(Ag._motion(DT, False, 1, {}))
    got = {}
    for canary in ga.CANARIES:
        arena = ga.GuardArena(canary)
        state = arena.view((12, B), torch.float64, "cuda")
        hist = arena.view((steps, 8, B), torch.float32, "cuda")
        state.copy_(state0)
        torch.ops.riab.agent_step_(state, hist, None, w_op, e_op, periodic, m, None, dev(z), None, None,
                                   dev(resample) if room == "polygon_hole" else None, ops.seed_arg(SEED), 0, ID0, steps)
        torch.cuda.synchronize()
        got.setdefault("state", arena.check(state, other=got.get("state")))
        got.setdefault("hist", arena.check(hist, other=got.get("hist")))
    resampled = 0
    for t in range(steps):
        st = orc.agent_step(oenv, st, DT, z[t, 0], z[t, 1], params={"speed_mean": float(Ag.speed_mean)},
                            resample_pos=resample[t].T if room == "polygon_hole" else None)
        resampled += int(st["bc_applied"].sum())
        h = got["hist"][t].astype(np.float64)
        np.testing.assert_allclose(h[0:2].T, st["pos"], rtol=2e-6, atol=2e-7)
        np.testing.assert_allclose(h[2:4].T, st["measured_velocity"], rtol=5e-6, atol=1e-6)
        np.testing.assert_allclose(h[4:6].T, st["head_direction"], rtol=5e-6, atol=1e-6)
        np.testing.assert_allclose(h[6], st["measured_rotational_velocity"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(h[7], st["distance_travelled"], rtol=1e-6)
    s = got["state"]
    for k, (a, b) in _STATE_ROWS.items():
        ref = np.asarray(st[k], dtype=np.float64).reshape(B, -1).T
        if k == "measured_rotational_velocity":
            np.testing.assert_allclose(s[a:b], ref, rtol=2e-6, atol=2e-6, err_msg=k)
        elif k == "distance_to_closest_wall":
            fin = np.isfinite(ref)
            np.testing.assert_allclose(s[a:b][fin], ref[fin], rtol=1e-9, err_msg=k)
        else:
            np.testing.assert_allclose(s[a:b], ref, rtol=1e-9, atol=1e-12, err_msg=k)
    if room == "polygon_hole":
        assert resampled >= int(in_hole.sum())           # the resample branch stored


# ---------------------------------------------------------------------------------------------------------------------
# (e) the streamed and planned forms: the package owns the buffers, the free tail of a history chunk is the guard
# ---------------------------------------------------------------------------------------------------------------------
TAIL = 4


class _Tail:
    """One DeviceHistory around a run of T rows: the two earlier rows are kept aside, T + TAIL free rows are made sure of
    and every free row of the newest chunk is filled with the canary."""

    def __init__(self, what, hist, T, canary):
        self.what, self.hist, self.T = what, hist, T
        assert len(hist) == 2, (what, hist.filled)
        self.before = hist.stack().clone()
        hist.preallocate(T + TAIL)
        self.start = hist.filled[-1]
        c = hist.chunks[-1]
        self.size = c.element_size()
        self.word = ga.canary_bits(canary, self.size)
        assert hist.caps[-1] - self.start >= T + TAIL
        c[self.start:].view(ga._INT[self.size]).fill_(self.word)

    def check(self):
        """the two earlier rows unchanged bit for bit, the T new rows free of the canary, every row behind them still
        canary -> the T new rows (NumPy)"""
        hist, T, s, what = self.hist, self.T, self.start, self.what
        assert len(hist) == 2 + T and hist.filled[-1] == s + T, (what, hist.filled)
        it = ga._INT[self.size]
        assert torch.equal(hist.stack()[:2].contiguous().view(it), self.before.view(it)), f"{what}: the earlier rows changed"
        rows = hist.chunks[-1][s:].view(it)
        touched = torch.nonzero(rows[T:].flatten() != self.word).flatten()
        assert len(touched) == 0, (f"{what}: {len(touched)} elements behind the run's rows were written, first at "
                                   f"{ga.coords(int(touched[0]) + T * rows[0].numel(), tuple(rows.shape))}")
        missing = torch.nonzero(rows[:T].flatten() == self.word).flatten()
        assert len(missing) == 0, (f"{what}: {len(missing)} elements of the run's rows were never written, first at "
                                   f"{ga.coords(int(missing[0]), tuple(rows.shape))}")
        return hist.chunks[-1][s:s + T].cpu().numpy()


def _place_ref(N, row, oenv, geom="euclidean"):
    pos = np.stack((row[0], row[1]), -1).astype(np.float64)
    return orc.place_cells(oenv, pos, N.place_cell_centres, N.place_cell_widths, wall_geometry=geom, max_fr=float(N.max_fr))


FORMS = ["one-kernel-T3", "one-kernel-T257", "populations", "chunks", "serial", "plan-step1", "plan-unfused"]


@pytest.mark.parametrize("canary", ga.CANARIES)
@pytest.mark.parametrize("spk", [False, True], ids=["nospikes", "spikes"])
@pytest.mark.parametrize("form", FORMS)
def test_streamed_and_planned_forms(riab, form, spk, canary):
    """256 agents and 9 cells (test_every_gated_table_slot's sizes; 260 agents for the plan that cannot fuse): simulate(2),
    then T rows into a chunk of T + 4 whose every element holds the canary.  `Agent.last_rate_stage_form()` /
    `riab_plan_info` say which form ran."""
    L = riab._lib
    T = 257 if form == "one-kernel-T257" else 3
    B = 260 if form == "plan-unfused" else 256
    walls = WALL if form == "chunks" else []
    np.random.seed(11)
    env, Ag = world(riab, B, {"walls": walls}, dt=0.01)
    oenv = orc.EnvSpec(walls=walls)
    np.random.seed(12)
    pops = [riab.PlaceCells(Ag, {"n": 9, "wall_geometry": "euclidean", "save_spikes": spk, "max_fr": 30.0})]
    if form == "populations":
        pops.append(riab.GridCells(Ag, {"n": 9, "save_spikes": spk, "max_fr": 30.0}))
    if form == "chunks":
        pops.append(riab.BoundaryVectorCells(Ag, {"n": 9, "save_spikes": spk, "max_fr": 30.0}))
    if form == "serial":
        tt = np.linspace(0, 3.0, 61)
        base = np.stack((0.5 + 0.35 * np.cos(2.1 * tt), 0.5 + 0.3 * np.sin(1.3 * tt + 0.4)), axis=-1)
        Ag.import_trajectory(times=tt, positions=base[:, None, :] + 0.05 * np.random.RandomState(9).uniform(-1, 1, (1, B, 2)))
    Ag.simulate(2)
    torch.cuda.synchronize()
    hists = [("agent", Ag._hist)] + [(f"{N.name} rates", N._hist_fr) for N in pops] + \
            ([(f"{N.name} spikes", N._hist_sp) for N in pops] if spk else [])
    tails = [_Tail(what, h, T, canary) for what, h in hists]
    if form == "populations":      # (9 cells never out-store a trajectory step: tell the choice that they do)
        L.check(L.lib.riab_streamer_configure(Ag._streamer, L.STREAMER_OPT_STEP_NS, 1), "configure")
        L.check(L.lib.riab_streamer_configure(Ag._streamer, L.STREAMER_OPT_LEAD_MBPS, 1), "configure")
    if form.startswith("plan"):
        plan = Ag.make_step_plan(capacity=T + TAIL)
        for _ in range(T):
            plan.step()
        info = plan.info()
        plan.close()
        torch.cuda.synchronize()
        assert info["fused_steps"] == (T if form == "plan-step1" else 0), info
        assert info["fused_enabled"] == (form == "plan-step1")
    else:
        Ag.simulate(T)
        torch.cuda.synchronize()
        assert Ag.last_rate_stage_form() == form.split("-T")[0], Ag.last_rate_stage_form()
        assert Ag.diagnostics["pipeline_timeouts"] == 0
    new = {tail.what: tail.check() for tail in tails}
    traj = new["agent"]
    for N in pops:
        fr = new[f"{N.name} rates"]
        for t in (0, T // 2, T - 1):
            pos = np.stack((traj[t, 0], traj[t, 1]), -1).astype(np.float64)
            if isinstance(N, riab.PlaceCells):
                assert_rates(fr[t], _place_ref(N, traj[t], oenv), scale=30.0)
            elif isinstance(N, riab.GridCells):
                assert_rates(fr[t], orc.grid_cells(pos, N.gridscales, N.phase_offsets, N.w, max_fr=30.0), scale=30.0, floor=1.0)
            else:
                assert_rates(fr[t], orc.bvc(pos, env.walls, N.tuning_distances, N.tuning_angles, N.sigma_distances, N.sigma_angles,
                                            max_fr=30.0), scale=30.0, floor=1.0)
        if spk:
            sp = new[f"{N.name} spikes"]
            assert (sp <= 1).all() and sp.sum() > 0
            for t in (0, T // 2, T - 1):                           # (rows 0.. are steps 3.. of the agent: two came before)
                uu = orc.spike_uniforms(SEED, 2 + t + 1, N.pop_id, 9, B, agent_id0=ID0)
                assert np.array_equal(sp[t].astype(bool), orc.spikes_f32(fr[t], uu, 0.01)), (N.name, t)


# ---------------------------------------------------------------------------------------------------------------------
# (f) positive control: no kernel changed, a legitimate in-arena write that lands in the back guard
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canary", ga.CANARIES)
def test_an_extra_row_is_caught_and_named(riab, canary):
    """riab_place_cells with n + 1 cells on a view declared for n: cell n of the only time row is row (1, 0, :) of the view's
    layout, the first B elements of the back guard.  `check` must fail, and name exactly that row."""
    from ratinabox_amd import ops
    L, n, B = riab._lib, 5, 4
    rows = rows_of(1, B)
    px, py = dev(rows["pos"][:, 0]), dev(rows["pos"][:, 1])
    rs = np.random.RandomState(3)
    tab = np.concatenate((rs.uniform(0.1, 0.9, (n + 1, 2)), np.full((n + 1, 1), -np.log2(np.e) / (2 * 0.2 ** 2))), 1)
    tab_t = dev(tab, np.float32)
    arena = ga.GuardArena(canary)
    rates = arena.view((1, n, B), torch.float32, "cuda")
    io = L.RiabRateIO()
    io.pos_x, io.pos_y, io.pos_ld, io.T, io.B = px.data_ptr(), py.data_ptr(), B, 1, B
    io.rates, io.dt, io.min_fr, io.max_fr = rates.data_ptr(), DT, 2.0, 12.0
    io.seed, io.step0, io.agent_id0, io.pop_id = SEED, STEP0, ID0, 3
    env = ops._env_struct(None, [0.0, 1.0, 0.0, 1.0, 1.0], False)
    rc = L.lib.riab_place_cells(env, io, L.ptr(tab_t), n + 1, L.PC_DESCRIPTIONS["gaussian"], L.GEOMETRIES["euclidean"], 0.2,
                                L.current_stream())
    assert rc == 0, L.strerror(rc)
    torch.cuda.synchronize()
    with pytest.raises(ga.GuardError) as e:
        arena.check(rates)
    assert e.value.kind == "back guard" and e.value.count == B
    assert e.value.first == (1, 0, 0) and e.value.last == (1, 0, B - 1)
    # ... and the rows the view was declared for are what n cells give
    want = orc.place_cells(orc.EnvSpec(), P(rows, 0), tab[:n, :2], np.full(n, 0.2), min_fr=2.0, max_fr=12.0)
    assert_rates(rates[0].cpu().numpy(), want, scale=10.0)
