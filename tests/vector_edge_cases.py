"""The cases at which tests/test_gpu_vector_edges.py drives csrc/riab_ovc.hip and HDCell::eval (csrc/riab_rate_cells.h),
built from fixed seeds: test infrastructure only, NumPy and the oracle only (tests/test_vector_edges_cpu.py checks the claims
the cases make about themselves without a GPU, so that the GPU tests cannot pass vacuously).

Every position, head direction, object and other-agent position is rounded to float32 and held as float64 (`f32`): the
oracle and the device then see the same numbers, and what is left between them is the kernel's own arithmetic.

A. narrow angular tunings (WIDTHS, degrees): about a third of the positions sit on the cells' preferred rays
   (`object - mu_d (cos, sin)(mu_t [+ head bearing])`, jittered by a fraction of the cell's sigmas), where the angular
   term's `cos - 1` cancels; head directions likewise sit near the preferred angles of the head-direction ring.
B. object counts M through the LDS regimes of `launch_ovc` (OBJECT_COUNTS; LDS_PER_OBJECT bytes each: up to 85 fit the
   default 64 KiB of dynamic LDS, 86..213 need the raised limit, 214 and more do not fit a CU's 160 KiB and are refused).
C. a periodic room with aspect 1.6 and scale 0.8, objects within 0.1 * scale of the edges.
D. degenerate geometry: an object exactly at a position, a head direction of (0, 0)."""
import numpy as np

from oracle import riab_oracle as orc

WIDTHS = (30.0, 10.0, 5.0, 3.0, 1.0)
RTOL = 1e-5
P_NARROW = 257
HD_N = 120

LDS_PER_OBJECT = 3 * 64 * 4            # stage A of ovc_kernel: (d, cos, sin) of 64 positions, float32
LDS_DEFAULT, LDS_CU = 64 * 1024, 160 * 1024
OBJECT_COUNTS = (1, 3, 4, 5, 85, 86, 213)
REFUSED_COUNTS = (214, 256, 257)
CELL_COUNTS = (1, 3, 4, 9)
POSITION_COUNTS = (1, 63, 64, 65, 257)

PERIODIC = dict(aspect=1.6, scale=0.8)


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def unit(angle):
    return np.stack((np.cos(angle), np.sin(angle)), axis=-1)


def tolerance(ref, scale=1.0, extra=0.0):
    """The project's check with the floor on: RTOL |ref| + RTOL (max_fr - min_fr) (+ a derived allowance)."""
    return RTOL * np.abs(ref) + RTOL * scale + extra + 1e-37


# ----------------------------------------------------------------------------- A. narrow tunings
def _on_rays(rs, objects, object_types, mu_d, mu_t, sg_d, sg_t, ttypes, hb, every=3):
    """Positions (len(hb), 2): every `every`-th one on the preferred ray of a cell (cells in turn) from an object of that
    cell's type, with a radial jitter of 0.3 sigma_d and an angular one of 0.5 sigma_angle; the others uniform in the
    middle of the room.  `hb`: head bearing of each position (zeros in the allocentric frame)."""
    P, n = len(hb), len(mu_d)
    pos = rs.uniform(0.1, 0.9, (P, 2))
    for k, p in enumerate(range(0, P, every)):
        c = k % n
        own = np.nonzero(np.asarray(object_types) == ttypes[c])[0]
        m = own[rs.randint(len(own))]
        r = mu_d[c] + 0.3 * sg_d[c] * rs.normal()
        ang = mu_t[c] + hb[p] + 0.5 * sg_t[c] * rs.normal()
        pos[p] = objects[m] - r * unit(ang)
    return pos


def narrow_ovc(width, ego):
    """ObjectVectorCells at one angular width: 24 cells, 5 objects of 2 types, 257 positions with head directions, two
    short interior walls (for `walls_occlude`).  dict(walls, objects, object_types, mu_d, mu_t, sg_d, sg_t, ttypes, pos, hd)."""
    rs = np.random.RandomState([41, int(width * 10), int(ego)])
    n = 24
    objects = f32(rs.uniform(0.3, 0.7, (5, 2)))
    object_types = np.array([0, 1, 0, 1, 0])
    mu_d, mu_t = rs.uniform(0.05, 0.25, n), rs.uniform(0, 2 * np.pi, n)
    sg_d, sg_t = rs.uniform(0.03, 0.1, n), np.full(n, np.radians(width))
    ttypes = rs.randint(0, 2, n)
    hb = rs.uniform(0, 2 * np.pi, P_NARROW)
    hd = f32(unit(hb))
    hb_seen = orc.get_angle(hd)         # the bearing both sides derive from the rounded vector
    pos = f32(_on_rays(rs, objects, object_types, mu_d, mu_t, sg_d, sg_t, ttypes, hb_seen if ego else np.zeros(P_NARROW)))
    walls = np.array([[[0.5, 0.3], [0.5, 0.45]], [[0.25, 0.6], [0.45, 0.6]]])
    return dict(walls=walls, objects=objects, object_types=object_types, mu_d=mu_d, mu_t=mu_t, sg_d=sg_d, sg_t=sg_t,
                ttypes=ttypes, pos=pos, hd=hd)


def ovc_reference(c, walls_occlude, ego, env=None, min_fr=0.0, max_fr=1.0):
    env = orc.EnvSpec(walls=c["walls"]) if env is None else env
    return orc.object_vector_cells(env, c["pos"], c["objects"], c["object_types"], c["mu_d"], c["mu_t"], c["sg_d"], c["sg_t"],
                                   c["ttypes"], walls_occlude=walls_occlude, head_direction=c["hd"] if ego else None,
                                   min_fr=min_fr, max_fr=max_fr)


FOV_DEFAULTS = dict(distance_range=[0.02, 0.4], angle_range=[0, 75], spatial_resolution=0.02)


def uniform_manifold():
    """(mu_d, mu_t, sg_d, sg_t) of `cell_arrangement="uniform_manifold"` at the reference's default field-of-view ranges."""
    from ratinabox_amd import utils
    return tuple(np.array(v) for v in utils.create_uniform_radial_assembly(**FOV_DEFAULTS))


def manifold_case(tuning, seed=43):
    """Egocentric cells on a manifold: 257 observers with head directions, each with ONE target of its own (`other`: what
    AgentVectorCells see); the first five targets double as the object list of the FieldOfViewOVCs case (types 0, 1, 0, 1, 0,
    cells tuned to type 0).  A third of the observers have their target on a cell's preferred ray."""
    mu_d, mu_t, sg_d, sg_t = tuning
    rs = np.random.RandomState(seed)
    P, n = P_NARROW, len(mu_d)
    hd = f32(unit(rs.uniform(0, 2 * np.pi, P)))
    hb = orc.get_angle(hd)
    other = f32(rs.uniform(0.3, 0.7, (P, 2)))
    object_types = np.array([0, 1, 0, 1, 0])
    pos_avc = rs.uniform(0.1, 0.9, (P, 2))
    pos_ovc = pos_avc.copy()
    cells = rs.permutation(n)
    for k, p in enumerate(range(0, P, 3)):
        c = cells[k % n]
        r = mu_d[c] + 0.3 * sg_d[c] * rs.normal()
        ang = mu_t[c] + hb[p] + 0.5 * sg_t[c] * rs.normal()
        pos_avc[p] = other[p] - r * unit(ang)
        pos_ovc[p] = other[(0, 2, 4)[k % 3]] - r * unit(ang)
    return dict(walls=np.zeros((0, 2, 2)), objects=other[:5], object_types=object_types, mu_d=mu_d, mu_t=mu_t, sg_d=sg_d,
                sg_t=sg_t, ttypes=np.zeros(n, dtype=int), pos=f32(pos_ovc), pos_avc=f32(pos_avc), other=other, hd=hd)


def avc_reference(c, walls_occlude=True, env=None):
    env = orc.EnvSpec() if env is None else env
    return orc.agent_vector_cells(env, c["pos_avc"], c["other"], c["mu_d"], c["mu_t"], c["sg_d"], c["sg_t"],
                                  walls_occlude=walls_occlude, head_direction=c["hd"])


def narrow_directions(width, n=HD_N, P=P_NARROW, speeds=False):
    """Direction vectors (P, 2) for a ring of `n` head-direction cells of spread `width`: every third within half a sigma
    of a cell's preferred angle, the others anywhere.  Unit vectors, or (`speeds`) velocities of 0.05 .. 0.4 m/s."""
    rs = np.random.RandomState([47, int(width * 10), int(speeds)])
    ang = rs.uniform(0, 2 * np.pi, P)
    pref = np.linspace(0, 2 * np.pi, n + 1)[:-1]
    for k, p in enumerate(range(0, P, 3)):
        ang[p] = pref[(7 * k) % n] + 0.5 * np.radians(width) * rs.normal()
    v = unit(ang)
    if speeds:
        v = v * rs.uniform(0.05, 0.4, (P, 1))
    return f32(v)


# ----------------------------------------------------------------------------- B. many objects
def object_types_for(M):
    """Types in the order Environment.add_object accepts them: object 1 is the ONLY one of type 1; every third object from
    the fourth on is of type 2, which no cell prefers; the rest are of type 0 (three types with uneven counts from M = 4)."""
    return np.array([1 if m == 1 else 2 if (m >= 3 and m % 3 == 0) else 0 for m in range(M)])


def tuning_types_for(n):
    """Cells prefer type 0, the last one (n > 1) type 1, whose single object is object 1; none prefers type 2."""
    t = np.zeros(n, dtype=int)
    if n > 1:
        t[-1] = 1
    return t


def interior_walls(seed=53, k=12):
    rs = np.random.RandomState(seed)
    a = rs.uniform(0.05, 0.95, (k, 2))
    ang, length = rs.uniform(0, np.pi, k), rs.uniform(0.15, 0.4, k)
    b = np.clip(a + length[:, None] * unit(ang), 0.02, 0.98)
    return f32(np.stack((a, b), axis=1))


def many_objects(M, n=9, P=257, seed=59):
    """M objects in a room with 12 interior walls; n cells with wide angular tunings (the sum over objects is the subject
    here); P positions with head directions."""
    rs = np.random.RandomState([seed, M])
    objects = f32(rs.uniform(0.03, 0.97, (M, 2)))
    pos_all, hd_all = f32(rs.uniform(0.02, 0.98, (max(POSITION_COUNTS), 2))), f32(unit(rs.uniform(0, 2 * np.pi, max(POSITION_COUNTS))))
    nmax = max(CELL_COUNTS)
    mu_d, mu_t = rs.uniform(0.05, 0.3, nmax), rs.uniform(0, 2 * np.pi, nmax)
    sg_d, sg_t = rs.uniform(0.08, 0.3, nmax), np.radians(rs.uniform(10, 30, nmax))
    return dict(walls=interior_walls(), objects=objects, object_types=object_types_for(M), mu_d=mu_d[:n], mu_t=mu_t[:n],
                sg_d=sg_d[:n], sg_t=sg_t[:n], ttypes=tuning_types_for(n), pos=pos_all[:P], hd=hd_all[:P])


def ovc_terms(c, walls_occlude, ego, env=None):
    """The oracle's own per-object terms (P, M, n), masked by type: what `orc.object_vector_cells` sums (its lines restated
    with the sum left out; tests/test_vector_edges_cpu.py checks that the sum of these IS the oracle's result)."""
    env = orc.EnvSpec(walls=c["walls"]) if env is None else env
    dist = orc.env_distances(env, c["pos"], c["objects"], "line_of_sight" if walls_occlude else "euclidean")
    vec = -1 * orc.env_vectors_between(env, c["pos"], c["objects"])
    bearing = orc.get_angle(vec.reshape(-1, 2)).reshape(dist.shape)
    if ego:
        bearing = bearing - orc.get_angle(c["hd"])[:, None]
    fr = orc.gaussian(dist[:, :, None], c["mu_d"][None, None], c["sg_d"][None, None]) * \
        orc.von_mises(bearing[:, :, None], c["mu_t"][None, None], c["sg_t"][None, None])
    return fr * (np.asarray(c["object_types"])[:, None] == np.asarray(c["ttypes"])[None, :])[None]


def sum_allowance(terms):
    """M * 2^-24 * sum over objects of |term| -> (n, P): the rounding of a sequential fp32 sum of M terms."""
    return (terms.shape[1] * 2.0 ** -24 * np.abs(terms).sum(axis=1)).T


def occlusion_margins(c):
    """(margin (P, M, W), blocked (P, M)): for every (position, object, wall) the distance of the strict-intersection
    decision `0 < l_a < 1 and 0 < l_b < 1` from flipping — |min(l_a, 1 - l_a, l_b, 1 - l_b)| (parallel pairs: inf)."""
    P, M = len(c["pos"]), len(c["objects"])
    segs = np.stack((np.repeat(c["pos"][:, None, :], M, 1), np.repeat(c["objects"][None, :, :], P, 0)), axis=-2).reshape(-1, 2, 2)
    l_a, l_b = orc.segment_intercepts(segs, c["walls"])
    with np.errstate(invalid="ignore"):
        m = np.minimum(np.minimum(l_a, 1 - l_a), np.minimum(l_b, 1 - l_b))
    margin = np.where(np.isfinite(m), np.abs(m), np.inf).reshape(P, M, -1)
    return margin, orc.segments_collide(segs, c["walls"]).any(axis=-1).reshape(P, M)


# ----------------------------------------------------------------------------- C. periodic rooms
def periodic_env():
    return orc.EnvSpec(boundary_conditions="periodic", **PERIODIC)


def periodic_case(seed=61, n=12, M=6, P=257):
    """Objects within 0.1 * scale of the edges of the 1.28 x 0.8 periodic room (the wrap uses `scale` on both axes, as the
    reference does), positions anywhere in it; `other`: one target per position, also near the edges."""
    rs = np.random.RandomState(seed)
    s, w = PERIODIC["scale"], PERIODIC["aspect"] * PERIODIC["scale"]

    def near_edges(k):
        x, y = rs.uniform(0, w, k), rs.uniform(0, s, k)
        e = rs.uniform(0.005, 0.1 * s, k)
        side = rs.randint(0, 4, k)
        x = np.where(side == 0, e, np.where(side == 1, w - e, x))
        y = np.where(side == 2, e, np.where(side == 3, s - e, y))
        return f32(np.stack((x, y), axis=-1))

    objects, other = near_edges(M), near_edges(P)
    pos = f32(np.stack((rs.uniform(0, w, P), rs.uniform(0, s, P)), axis=-1))
    hd = f32(unit(rs.uniform(0, 2 * np.pi, P)))
    return dict(walls=np.zeros((0, 2, 2)), objects=objects, object_types=np.array([0, 1, 0, 1, 0, 1][:M]),
                mu_d=rs.uniform(0.05, 0.3, n), mu_t=rs.uniform(0, 2 * np.pi, n), sg_d=rs.uniform(0.08, 0.2, n),
                sg_t=np.radians(rs.uniform(10, 30, n)), ttypes=rs.randint(0, 2, n), pos=pos, pos_avc=pos, other=other, hd=hd)


def wrap_report(c, targets):
    """(fraction of (position, target) pairs wrapped on some axis, min | |v| - scale/2 |) for targets (M, 2) seen from
    every position, or (P, 2) seen one per position."""
    s = PERIODIC["scale"]
    v = c["pos"][:, None, :] - targets[None] if len(targets) != len(c["pos"]) else (c["pos"] - targets)[:, None, :]
    a = np.abs(v)
    return float((a > s / 2).any(axis=-1).mean()), float(np.abs(a - s / 2).min())


# ----------------------------------------------------------------------------- D. degenerate geometry
def degenerate_case(seed=67, n=8, P=64):
    """Every fourth position IS an object (d = 0, bearing = atan2(0, 1e-6) = 0); every fourth (offset by two) head direction
    is (0, 0) (get_angle: atan2(0, 1e-6) = 0)."""
    rs = np.random.RandomState(seed)
    objects = f32(rs.uniform(0.2, 0.8, (4, 2)))
    pos, hd = f32(rs.uniform(0.1, 0.9, (P, 2))), f32(unit(rs.uniform(0, 2 * np.pi, P)))
    pos[0::4] = objects[np.arange(len(pos[0::4])) % 4]
    hd[2::4] = 0.0
    return dict(walls=np.zeros((0, 2, 2)), objects=objects, object_types=np.array([0, 0, 1, 1]), mu_d=rs.uniform(0.0, 0.2, n),
                mu_t=rs.uniform(0, 2 * np.pi, n), sg_d=rs.uniform(0.05, 0.2, n), sg_t=np.radians(rs.uniform(10, 30, n)),
                ttypes=rs.randint(0, 2, n), pos=pos, hd=hd)
