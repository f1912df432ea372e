"""The OU rate noise of Neurons.update (noise_std > 0) against the float64 oracle (run with `-m gpu` on an MI355X).

The device draws the noise in `noise_kernel` (csrc/riab_rates.hip): Philox4x32-7 + Box-Muller in fp32, then the OU
recurrence in fp32.  `orc.noise_normals` regenerates the normals on the host from the same counters and
`orc.ou_noise_path` runs the recurrence in float64 on the kernel's own fp32 constants, so every path is pinned to
something outside the product, not only to another product path.

Tolerances:
  * one step from zero, the output is sigma_dt * z: z is compared at the motion stream's tolerances (rtol 1e-5, atol
    2e-5; tests/test_gpu_parity.py): the Philox words are bit-exact, log / sin / cos are the fp32 hardware
    approximations (~1e-6 of z) and z reaches ~6;
  * several steps: |x_dev - x_ref| <= 1e-5 |x_ref| + 1e-4 * noise_std.  Per step the device adds sigma_dt * dz, dz ~
    1e-6 * |z|, plus one fp32 rounding of x (6e-8 |x|).  Both decay by a = 1 - dt/tau per step, so the sum stays at
    ~sigma_dt * 1e-6 * 6 / sqrt(1 - a^2) + 6e-8 |x| / (1 - a) <= noise_std * (1e-5 + 6e-8 * 6 / 0.01): below 1e-4 *
    noise_std for dt/tau >= 0.01 (sigma_dt = noise_std * sqrt(2 dt/tau), |x| < 6 noise_std);
  * rates of a noisy population = its noiseless twin's fp32 rates + the oracle's path: the same, plus rtol 1e-5 on the
    rate (the fp32 sum rounds once);
  * spikes: bit-exact (orc.spikes_f32 on the kernel's own noisy fp32 rates and orc.spike_uniforms)."""
import numpy as np
import pytest
import torch

from oracle import riab_oracle as orc
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

SEED = (0xC0FFEE << 32) | 0x2545F491   # both key words nonzero
DT = 0.02
B_RAGGED, AID0 = 70, 1024                # an agent axis that is not a multiple of 4, on a shard at offset 1024


@pytest.fixture(scope="module")
def riab():
    assert torch.cuda.is_available(), "these tests need the GPU"
    import ratinabox_amd
    return ratinabox_amd


def f32(x):
    return float(np.float32(x))


def assert_noise(got, ref, noise_std, rates=None, what=""):
    """|got - ref| <= 1e-5 |rate or ref| + 1e-4 noise_std (derivation: module docstring)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = np.abs(ref) if rates is None else np.maximum(np.abs(ref), np.abs(rates))
    err = np.abs(got - ref)
    bad = ~(err <= 1e-5 * scale + 1e-4 * noise_std)
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} outside tolerance, worst abs err {np.nanmax(err):.3e}"


# ----------------------------------------------------------------------------- the raw entry point
# (n, B, T, agent_id0, pop_id, dt/tau): every listed value of each axis at least once; n = 65537 is more cells than
# the 65535 rows of workgroups the launch puts on the grid's y axis
RAW_CASES = [
    (1, 4, 1, 0, 0, 0.1),
    (3, 68, 5, 4, 7, 0.5),
    (17, 1100, 64, 1 << 20, 255, 0.01),
    (1000, 4100, 1, 4, 255, 0.1),
    (1000, 68, 64, 0, 7, 0.1),
    (65537, 4, 5, 1 << 20, 0, 0.5),
    (65537, 68, 1, 0, 255, 0.01),
    (3, 4100, 64, 0, 7, 0.5),
    (17, 4, 64, 4, 0, 0.01),
    (1, 1100, 5, 1 << 20, 7, 0.1),
    (17, 4100, 5, 0, 255, 0.1),
]


@pytest.mark.parametrize("n,B,T,aid0,pop_id,ratio", RAW_CASES)
def test_raw_noise_is_the_oracles_ou_path(riab, n, B, T, aid0, pop_id, ratio):
    """riab_neuron_noise on zeroed noise and rates: the rates rows are the OU path itself, the noise buffer its last
    state.  step0 is 3 below 2^32 (the counter word wraps inside the call), the seed's high word is nonzero."""
    _L = riab._lib
    noise_std, tau = 0.7, 0.25
    theta_dt, sigma_dt = f32(ratio), f32(np.sqrt(2 * noise_std**2 / (tau * ratio * tau)) * ratio * tau)
    step0 = (1 << 32) - 3
    guard = 64
    noise = torch.zeros(n * B + guard, dtype=torch.float32, device="cuda")
    rates = torch.zeros(T * n * B + guard, dtype=torch.float32, device="cuda")
    noise[n * B:] = 7.0
    rates[T * n * B:] = 7.0
    rc = _L.lib.riab_neuron_noise(_L.ptr(noise), _L.ptr(rates), None, n, B, T, theta_dt, sigma_dt, SEED, step0, pop_id,
                                  aid0, _L.current_stream())
    assert rc == 0, _L.strerror(rc)
    torch.cuda.synchronize()
    # nothing written past the buffers
    assert bool((noise[n * B:] == 7.0).all()) and bool((rates[T * n * B:] == 7.0).all())
    x = rates[:T * n * B].view(T, n, B).cpu().numpy().astype(np.float64)
    z = np.stack([orc.noise_normals(SEED, step0 + t, pop_id, n, B, agent_id0=aid0) for t in range(T)])
    np.testing.assert_allclose(x[0] / sigma_dt, z[0], rtol=1e-5, atol=2e-5)
    ref = orc.ou_noise_path(z, theta_dt, sigma_dt)
    assert_noise(x, ref, noise_std, what=f"n={n} B={B} T={T}")
    assert np.array_equal(noise[:n * B].view(n, B).cpu().numpy(), x[-1].astype(np.float32))


def test_device_noise_follows_the_ou_law(riab):
    """The production stream (in-kernel Philox), 2^18 lanes x 200 steps from zero, for dt/tau in {0.01, 0.1, 0.5}:
    per-step sample mean and variance against the exact Var x_t = sigma_dt^2 (1 - a^2t) / (1 - a^2), a = 1 - dt/tau,
    and the lag-1 / lag-10 regression Cov(x_t, x_t+k) / Var x_t against a^k, each within 5 standard errors."""
    _L = riab._lib
    n, B, T = 64, 4096, 200
    N = n * B
    noise_std, tau = 0.5, 0.2
    for ratio in (0.01, 0.1, 0.5):
        dt = ratio * tau
        theta_dt, sigma_dt = f32(ratio), f32(np.sqrt(2 * noise_std**2 / (tau * dt)) * dt)
        a = 1 - theta_dt
        noise = torch.zeros((n, B), dtype=torch.float32, device="cuda")
        rates = torch.zeros((T, n, B), dtype=torch.float32, device="cuda")
        rc = _L.lib.riab_neuron_noise(_L.ptr(noise), _L.ptr(rates), None, n, B, T, theta_dt, sigma_dt, SEED, 12345, 3, 0,
                                      _L.current_stream())
        assert rc == 0, _L.strerror(rc)
        x = rates.view(T, N).double()
        t = np.arange(1, T + 1)
        var = sigma_dt**2 * (1 - a ** (2 * t)) / (1 - a**2)
        m2 = (x * x).mean(1).cpu().numpy()
        mean = x.mean(1).cpu().numpy()
        assert np.all(np.abs(m2 / var - 1) < 5 * np.sqrt(2 / N)), (ratio, np.max(np.abs(m2 / var - 1)))
        assert np.all(np.abs(mean) < 5 * np.sqrt(var / N)), ratio
        if ratio == 0.5:   # stationary by the last steps: noise_std^2 * 2 / (2 - dt/tau)
            assert abs(m2[-1] / (noise_std**2 * 2 / (2 - ratio)) - 1) < 5 * np.sqrt(2 / N)
        for k in (1, 10):
            i = T - 1 - k
            beta = float((x[i] * x[i + k]).sum() / (x[i] * x[i]).sum())
            se = np.sqrt((var[i + k] - a ** (2 * k) * var[i]) / (N * var[i]))
            assert abs(beta - a**k) < 5 * se, (ratio, k, beta, a**k)


# ----------------------------------------------------------------------------- every path, every noisy population kind
NOISE = dict(noise_std=0.4, noise_coherence_time=0.1)   # dt/tau = 0.2
NOISE_SLOW = dict(noise_std=0.25, noise_coherence_time=0.5)
WALLS = [[[0.5, 0.2], [0.5, 0.6]]]
OBJECTS = [[0.3, 0.7], [0.8, 0.3]]


def _kinds(riab):
    """(name, constructor(Ag, params)) of every Neurons class that takes noise_std > 0 and lives on one Agent."""
    return [
        ("PlaceCells", lambda Ag, p: riab.PlaceCells(Ag, dict(p, n=9, max_fr=20.0))),
        ("GridCells", lambda Ag, p: riab.GridCells(Ag, dict(p, n=6, max_fr=15.0))),
        ("HeadDirectionCells", lambda Ag, p: riab.HeadDirectionCells(Ag, dict(p, n=5, max_fr=15.0))),
        ("VelocityCells", lambda Ag, p: riab.VelocityCells(Ag, dict(p, max_fr=15.0))),
        ("SpeedCell", lambda Ag, p: riab.SpeedCell(Ag, dict(p, max_fr=15.0))),
        ("BoundaryVectorCells", lambda Ag, p: riab.BoundaryVectorCells(Ag, dict(p, n=6, max_fr=15.0))),
        ("FieldOfViewBVCs", lambda Ag, p: riab.FieldOfViewBVCs(Ag, dict(p, max_fr=15.0))),
        ("ObjectVectorCells", lambda Ag, p: riab.ObjectVectorCells(Ag, dict(p, n=4, max_fr=15.0))),
        ("FieldOfViewOVCs", lambda Ag, p: riab.FieldOfViewOVCs(Ag, dict(p, object_tuning_type=0, max_fr=15.0))),
        ("RandomSpatialNeurons", lambda Ag, p: riab.RandomSpatialNeurons(Ag, dict(p, n=3, wall_geometry="euclidean",
                                                                                 max_fr=15.0))),
    ]


def _world(riab, task=False):
    """An agent of B_RAGGED agents at AID0 with, for every kind, a noisy population and its noiseless twin (same tuning:
    same NumPy seed), and a FeedForwardLayer pair reading a noiseless PlaceCells layer.  -> (Ag, env, [(noisy, twin)])"""
    params = {"walls": WALLS, "objects": OBJECTS}
    if task:
        from ratinabox_amd.contribs.TaskEnvironment import SpatialGoalEnvironment
        env = SpatialGoalEnvironment(params=params, possible_goal_positions=[[0.2, 0.25], [0.8, 0.7]], seed=3, dt=DT)
    else:
        env = riab.Environment(params)
    np.random.seed(0)
    Ag = riab.Agent(env, {"n_agents": B_RAGGED, "dt": DT, "seed": SEED, "agent_id0": AID0})
    pairs = []
    for k, (name, make) in enumerate(_kinds(riab)):
        noise = NOISE if k % 2 == 0 else NOISE_SLOW
        np.random.seed(100 + k)
        N = make(Ag, dict(noise, name=name + "_noisy"))
        np.random.seed(100 + k)
        W = make(Ag, {"name": name + "_twin"})
        pairs.append((N, W))
    np.random.seed(7)
    inp = riab.PlaceCells(Ag, {"n": 12, "name": "ff_input"})
    np.random.seed(8)
    N = riab.FeedForwardLayer(Ag, dict(NOISE, n=5, input_layers=[inp], name="ff_noisy", max_fr=15.0))
    np.random.seed(8)
    W = riab.FeedForwardLayer(Ag, dict(n=5, input_layers=[inp], name="ff_twin", max_fr=15.0))
    pairs.append((N, W))
    if task:
        env.add_agents(Ag)
    return Ag, env, pairs


def _check_pairs(Ag, pairs, T):
    """Every noisy population == twin + oracle OU path (rows 0..T-1 = steps 1..T of a fresh agent), its noise state
    the path's end, its spikes the oracle rule on its own rates."""
    B = Ag._B
    for N, W in pairs:
        assert N.pop_id != W.pop_id and N.n == W.n
        fr, sp = (h.cpu().numpy() for h in N.get_history_tensors())
        frw = W.get_history_tensors()[0].cpu().numpy()
        assert fr.shape[0] == T, (N.name, fr.shape)
        Bp, n = N._Bp, int(N.n)
        theta_dt, sigma_dt = (f32(c) for c in N._noise_constants(DT))
        z = np.stack([orc.noise_normals(SEED, t + 1, N.pop_id, n, Bp, agent_id0=AID0) for t in range(T)])
        x = orc.ou_noise_path(z, theta_dt, sigma_dt)[:, :, :B]
        rates_w = frw[:, :, :B].astype(np.float64)
        assert np.isfinite(rates_w).all(), W.name
        assert_noise(fr[:, :, :B], rates_w + x, N.noise_std, rates=rates_w, what=N.name)
        assert_noise(N.noise, x[-1], N.noise_std, what=N.name + " state")
        assert np.abs(x).max() > 0.1 * N.noise_std
        for t in range(T):
            u = orc.spike_uniforms(SEED, t + 1, N.pop_id, n, Bp, agent_id0=AID0)[:, :B]
            assert np.array_equal(sp[t][:, :B].astype(bool), orc.spikes_f32(fr[t][:, :B], u, DT)), (N.name, t)
    assert sum(int(N.get_history_tensors()[1].sum()) for N, _ in pairs) > 0


T_PATHS = 7   # (> Agent.AUTO_AFTER: the automatic plan serves the last steps)


@pytest.mark.parametrize("path", ["eager", "simulate1", "simulate5", "plan", "auto", "task"])
def test_noisy_populations_every_path(riab, path):
    Ag, env, pairs = _world(riab, task=(path == "task"))
    T = T_PATHS
    if path in ("eager", "auto"):
        Ag._auto_enabled = path == "auto"
        for _ in range(T):
            Ag.update()
            for N in Ag.Neurons:
                N.update()
        assert (type(Ag._plan).__name__ == "AutoStepper") == (path == "auto")
    elif path.startswith("simulate"):
        Ag.simulate(T, chunk=int(path[len("simulate"):]))
    elif path == "plan":
        plan = Ag.make_step_plan(capacity=4)
        for _ in range(T):
            plan.step()
    else:
        plan = env.make_step_plan(auto_reset=False)
        for _ in range(T):
            plan.step(1)
    torch.cuda.synchronize()
    assert Ag._step_index == T
    _check_pairs(Ag, pairs, T)


# ----------------------------------------------------------------------------- sharding
def test_noise_is_shard_invariant(riab):
    """B = 1024 agents == two Agents of 512 at agent_id0 0 and 512 with the same seed and starting state: the noisy
    rates, noise states and spikes bit for bit."""
    T = 5

    def world(B, aid0, st0=None):
        np.random.seed(4)
        Ag = riab.Agent(riab.Environment(), {"n_agents": B, "dt": DT, "seed": SEED, "agent_id0": aid0})
        Ag._auto_enabled = False
        if st0 is not None:
            for k in gu.PRE_SLICES:
                setattr(Ag, k, st0[k][aid0:aid0 + B])
        np.random.seed(5)
        PCs = riab.PlaceCells(Ag, {"n": 21, "max_fr": 20.0, **NOISE})
        return Ag, PCs

    Ag, P = world(1024, 0)
    st0 = {k: np.array(getattr(Ag, k)) for k in gu.PRE_SLICES}
    halves = [world(512, 0, st0), world(512, 512, st0)]
    for A, N in [(Ag, P)] + halves:
        for _ in range(T):
            A.update()
            N.update()
    torch.cuda.synchronize()
    fr = P.history["firingrate"]
    sp = P.history["spikes"]
    for h, (A, N) in enumerate(halves):
        s = slice(512 * h, 512 * (h + 1))
        assert np.array_equal(A.pos, Ag.pos[s])
        assert np.array_equal(N.noise, P.noise[:, s])
        assert np.array_equal(N.history["firingrate"], fr[:, :, s])
        assert np.array_equal(N.history["spikes"], sp[:, :, s])
    assert np.std(P.noise) > 0.1 * NOISE["noise_std"]


# ----------------------------------------------------------------------------- a plan stepped at another dt
def test_plan_step_at_new_dt_takes_the_noise_with_it(riab):
    """plan.step(dt=d2) on a plan built at d1 == `Ag.update(dt=d2); N.update()`: the populations' OU constants follow
    the step's dt (Neurons.update reads Agent.dt), as the spike rule does."""
    d1, d2 = DT, 0.005

    def world():
        np.random.seed(12)
        Ag = riab.Agent(riab.Environment({"walls": WALLS}), {"n_agents": B_RAGGED, "dt": d1, "seed": SEED,
                                                            "agent_id0": AID0})
        Ag._auto_enabled = False
        np.random.seed(13)
        pcs = riab.PlaceCells(Ag, {"n": 10, "max_fr": 30.0, **NOISE})
        bvc = riab.BoundaryVectorCells(Ag, {"n": 4, "max_fr": 30.0, **NOISE_SLOW})
        return Ag, [pcs, bvc]

    A1, P1 = world()
    for dt in (d1, d1, d2, d2, d2):
        A1.update(dt=dt)
        for N in P1:
            N.update()
    A2, P2 = world()
    plan = A2.make_step_plan(capacity=8)
    for dt in (d1, d1, d2, d2, d2):
        plan.step(dt=dt)
    torch.cuda.synchronize()
    assert np.array_equal(A2.pos, A1.pos)
    for a, b in zip(P1, P2):
        assert np.array_equal(b.noise, a.noise), a.name
        assert np.array_equal(b.history["firingrate"], a.history["firingrate"]), a.name
        assert np.array_equal(b.history["spikes"], a.history["spikes"]), a.name
    # and the eager side is the oracle's: the OU constants of d2 from the third step on
    N = P1[0]
    Bp, n = N._Bp, int(N.n)
    z = np.stack([orc.noise_normals(SEED, t + 1, N.pop_id, n, Bp, agent_id0=AID0) for t in range(5)])
    c1, c2 = ([f32(c) for c in N._noise_constants(d)] for d in (d1, d2))
    x = orc.ou_noise_path(z[:2], *c1)
    x = np.concatenate((x, orc.ou_noise_path(z[2:], *c2, x0=x[-1])))
    assert_noise(N.noise, x[-1][:, :A1._B], N.noise_std, what="eager at d2")


# ----------------------------------------------------------------------------- many populations
def test_population_256_has_streams_of_its_own(riab):
    """257 one-cell noisy, spiking populations on one agent: population 256 draws neither the noise nor the spike
    uniforms of population 0 (a stream tag masked to 8 bits gave it exactly those); each matches the oracle's own
    stream for its pop_id."""
    B, T = 256, 2
    np.random.seed(21)
    Ag = riab.Agent(riab.Environment(), {"n_agents": B, "dt": DT, "seed": SEED})
    Ag._auto_enabled = False
    centre = np.array([[0.5, 0.5]])
    pops = [riab.PlaceCells(Ag, {"place_cell_centres": centre, "widths": 2.0, "max_fr": 40.0, "save_history": True,
                                 **NOISE}) for _ in range(257)]
    assert [p.pop_id for p in (pops[0], pops[256])] == [0, 256]
    for _ in range(T):
        Ag.update()
        for N in pops:
            N.update()
    torch.cuda.synchronize()
    a, b = pops[0], pops[256]
    assert not np.array_equal(a.noise, b.noise)
    fa, fb = a.history["firingrate"], b.history["firingrate"]
    assert not np.array_equal(fa, fb)
    for N in (a, b, pops[255]):
        theta_dt, sigma_dt = (f32(c) for c in N._noise_constants(DT))
        z = np.stack([orc.noise_normals(SEED, t + 1, N.pop_id, 1, B) for t in range(T)])
        assert_noise(N.noise, orc.ou_noise_path(z, theta_dt, sigma_dt)[-1], N.noise_std, what=N.name)
        fr, sp = (h.cpu().numpy() for h in N.get_history_tensors())
        for t in range(T):
            u = orc.spike_uniforms(SEED, t + 1, N.pop_id, 1, B)
            assert np.array_equal(sp[t][:, :B].astype(bool), orc.spikes_f32(fr[t][:, :B], u, DT)), (N.pop_id, t)
    assert not np.array_equal(orc.spike_uniforms(SEED, 1, 0, 1, B), orc.spike_uniforms(SEED, 1, 256, 1, B))
    assert a.history["spikes"].sum() > 0
