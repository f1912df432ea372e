"""The cases at which tests/test_gpu_bvc_rays.py drives `bvc_kernel` (csrc/riab_bvc.hip) through its C entry point, with
the ray stage made visible by the ABI's `ray_out`: test infrastructure only — NumPy and the oracle
(tests/test_bvc_rays_cpu.py checks without a GPU what the cases claim about themselves, so that the GPU tests cannot pass
vacuously).

Every position and head direction is rounded to float32 and held as float64 (`f32`): the oracle and the device then see
the same numbers, and what is left between them is the kernel's own arithmetic.

* direction tables (TABLES) and rooms (ROOMS), each named after the branch of stage A it reaches; `kernel_paired`,
  `kernel_box_edges`, `kernel_box4`, `kernel_split` and `kernel_kp` restate the kernel's own rules for those branches;
* `bvc_tables`: the device tables, built with the expressions of `BoundaryVectorCells._call`;
* `oracle_rays`: `oracle.bvc_ray_distances` with the wall it chose and the line parameters it chose on (the distances
  are the oracle's: the CPU test asserts it);
* `ray_tolerance`, `exclusions`: the bound of a ray and the pairs that may be left out, from the inputs alone;
* `kernel_rays`: stage A restated in NumPy float64 (before and after the on-edge fix) — what the CPU test compares with
  the oracle so that the bound and the exclusions are tried before a device is;
* `stage_b_reference` / `stage_b_float32`: the float64 sum `oracle.bvc` forms over given distances, and its float32
  restatement that sizes the stage-B tolerance."""
import numpy as np

from oracle import riab_oracle as orc

LOG2E = 1.4426950408889634
EPS64 = 2.0 ** -52
NEAR = 1e-9                       # a decision of the oracle closer than this to flipping may be left out
FALLBACK_BIG = 1e3                # a miss whose wall 0 is within 1e-3 rad of parallel to the ray
CAP = 0.005                       # of the pairs of a case; 0 for positions strictly inside
ROWS = dict(T=3, B=68, pos_ld=72)  # tiles straddle time rows, the leading dimension differs from B
BVC_WINDOW_SHARE = 1e-6

MAZE = [[[.2, 0], [.2, .4]], [[.4, 1], [.4, .6]], [[.6, 0], [.6, .4]], [[.8, 1], [.8, .6]], [[.3, .5], [.7, .5]]]
EDGE_POSITIONS = np.array([[0.0, 0.5], [1.0, 0.25], [0.5, 0.0], [0.5, 1.0]])
OUTSIDE_POSITIONS = np.array([[-0.25, 0.375], [1.5, 1.25]])


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# ----------------------------------------------------------------------------- direction tables
def _reference_table(dtheta):
    return orc.bvc_test_angles(dtheta)


def _moved_table():
    """The reference table with one entry moved by 1e-9: it fails the kernel's opposite check (1e-12)."""
    angles, dirs = orc.bvc_test_angles(2)
    dirs = dirs.copy()
    dirs[2, 0] += 1e-9
    return angles, dirs


def _scrambled_table():
    """16 directions in no particular order, the exact axis directions (+-1, 0), (0, +-1) among them."""
    rs = np.random.RandomState(71)
    angles = np.concatenate(([0.0, np.pi / 2, np.pi, 3 * np.pi / 2], rs.uniform(0, 2 * np.pi, 12)))
    dirs = np.stack((np.cos(angles), np.sin(angles)), axis=-1)
    dirs[:4] = [[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]]
    order = rs.permutation(16)
    return angles[order], dirs[order]


# name -> (builder, K, paired, what it reaches)
TABLES = {
    "K180": (lambda: _reference_table(2), 180, True, "reference table: paired, KB = 4, cast_single(1 + m - np, np)"),
    "K51": (lambda: _reference_table(7), 51, False, "odd K: unpaired, Kp = 52 pad row, clamped last batch"),
    "K12": (lambda: _reference_table(30), 12, False, "np = 5 < 8: unpaired although even"),
    "K18": (lambda: _reference_table(20), 18, True, "np = 8: the smallest paired table"),
    "K360": (lambda: _reference_table(1), 360, True, "the maximum: LDS above 64 KB"),
    "K1": (lambda: _reference_table(360), 1, False, "single direction"),
    "K7": (lambda: _reference_table(51), 7, False, "not a multiple of 4"),
    "K180moved": (_moved_table, 180, False, "fails the opposite check: one ray at a time"),
    "K16scrambled": (_scrambled_table, 16, False, "no particular order, exact axis directions"),
}


def table(name):
    angles, dirs = TABLES[name][0]()
    return np.array(angles, dtype=np.float64), np.array(dirs, dtype=np.float64)


def kernel_kp(K):
    return (K + 3) // 4 * 4


def kernel_paired(dirs):
    """bvc_kernel's `paired`: K even, np = K - 1 - K/2 >= 8, and entries j and j + K/2 opposite to 1e-12 for j = 1 .. np."""
    K = len(dirs)
    m = K >> 1
    n_pairs = K - 1 - m
    if K & 1 or n_pairs < 8:
        return False
    j = np.arange(1, n_pairs + 1)
    return bool((np.abs(dirs[j] + dirs[j + m]) <= 1e-12).all())


# ----------------------------------------------------------------------------- rooms
L_ROOM = [[1, 0.5], [0.5, 0.5], [0.5, 1], [0, 1], [0, 0], [1, 0]]     # wall 0 runs from (0.5, 0.5) to (1, 0.5): the notch


def _comb():
    import bench
    return bench.comb_walls(60)


def room(name):
    """dict(walls (Nw, 2, 2) as handed to the ABI, extent, polygon, n_boundary, inside(rs, P) -> positions strictly inside,
    on_walls: positions on interior walls and at their free ends)."""
    def box_inside(rs, P):
        return f32(rs.uniform(0.01, 0.99, (P, 2)))

    def l_inside(rs, P):
        p = rs.uniform(0.01, 0.99, (4 * P, 2))
        return f32(p[~((p[:, 0] > 0.49) & (p[:, 1] > 0.49))][:P])

    maze_on = np.array([[0.5, 0.5], [0.4375, 0.5], [0.3, 0.5], [0.7, 0.5], [0.2, 0.25], [0.2, 0.4], [0.8, 0.6], [0.6, 0.125]])
    if name in ("box", "box_polygon"):
        env = orc.EnvSpec()
        return dict(walls=env.walls, extent=env.extent, polygon=int(name.endswith("polygon")), n_boundary=4,
                    inside=box_inside, on_walls=np.zeros((0, 2)))
    if name in ("maze", "maze_polygon"):
        env = orc.EnvSpec(walls=MAZE)
        return dict(walls=env.walls, extent=env.extent, polygon=int(name.endswith("polygon")), n_boundary=4,
                    inside=box_inside, on_walls=f32(maze_on))
    if name == "comb64":
        env = orc.EnvSpec(walls=_comb())
        x = 1 / 31
        return dict(walls=env.walls, extent=env.extent, polygon=0, n_boundary=4, inside=box_inside,
                    on_walls=f32([[x, 0.25], [x, 0.3], [x, 0.4], [2 * x, 0.7], [2 * x, 0.5]]))
    if name == "lroom":
        env = orc.EnvSpec(boundary=L_ROOM)
        return dict(walls=env.walls, extent=env.extent, polygon=1, n_boundary=6, inside=l_inside, on_walls=np.zeros((0, 2)))
    if name == "interior_first":
        # two interior walls BEFORE the room's edges in the table: the rectangular room is announced (polygon = 0) but
        # the kernel's check of the first four walls fails
        env = orc.EnvSpec(walls=MAZE)
        walls = np.concatenate((env.walls[4:6], env.walls[:4], env.walls[6:]))
        return dict(walls=walls, extent=env.extent, polygon=0, n_boundary=4, inside=box_inside, on_walls=f32(maze_on))
    raise KeyError(name)


# name -> (the four-edge check holds, the path)
ROOMS = {
    "box": (True, "box fast path"),
    "maze": (True, "fast path, then the full test for interior walls"),
    "box_polygon": (False, "general path: the same table described as a polygon"),
    "maze_polygon": (False, "general path: the same table described as a polygon"),
    "comb64": (True, "64 walls"),
    "lroom": (False, "wall 0 is not a box edge"),
    "interior_first": (False, "rect_room set, four-edge check fails"),
}


def kernel_box_edges(r):
    """bvc_kernel's check of the first four walls: a rectangular room is announced, and the walls are axis-aligned, on the
    extent and span it, two of each orientation."""
    walls, (e0, e1, e2, e3) = np.asarray(r["walls"]).reshape(-1, 4), r["extent"]
    if r["polygon"] or len(walls) < 4:
        return False
    tol = 1e-9 * ((e1 - e0) + (e3 - e2))
    nh = nv = 0
    for ax, ay, bx, by in walls[:4]:
        if ay == by and ax != bx:
            nh += 1
            if not ((ay == e2 or ay == e3) and min(ax, bx) <= e0 + tol and max(ax, bx) >= e1 - tol):
                return False
        elif ax == bx and ay != by:
            nv += 1
            if not ((ax == e0 or ax == e1) and min(ay, by) <= e2 + tol and max(ay, by) >= e3 - tol):
                return False
        else:
            return False
    return nh == 2 and nv == 2


def kernel_box4(r, pos):
    """Per tile of 64 positions (in launch order): does the tile take the box fast path?"""
    pos = np.asarray(pos).reshape(-1, 2)
    e0, e1, e2, e3 = r["extent"]
    inside = (pos[:, 0] > e0) & (pos[:, 0] < e1) & (pos[:, 1] > e2) & (pos[:, 1] < e3)
    ok = kernel_box_edges(r)
    return np.array([ok and bool(inside[s:s + 64].all()) for s in range(0, len(pos), 64)])


def kernel_split(n, P):
    """launch_bvc's grid.y: the workgroups that share a tile's cell groups."""
    tiles, n_groups, split = (P + 63) // 64, (n + 3) // 4, 1
    while split < 8 and tiles * split * 2 <= 512 and split * 2 * 8 <= n_groups:
        split *= 2
    return split


# ----------------------------------------------------------------------------- the ray cases
def _layout(pos, T, B):
    assert len(pos) == T * B
    return f32(pos).reshape(T, B, 2)


def _mixed(r, rs, P):
    """Interior positions with a tile of special ones in the middle: on interior walls and at their free ends, and the
    two outside positions (launch positions 64 ..: one tile leaves the fast path, the others stay on it)."""
    pos = r["inside"](rs, P)
    special = np.concatenate((r["on_walls"], OUTSIDE_POSITIONS))
    pos[70:70 + len(special)] = special
    return pos


def ray_cases():
    """[(id, dict(room, table, pos (T, B, 2), pos_ld, n, cap, inside))]: every table in every room at strictly interior
    positions (cap 0), and the positions that are not: on the edges, on interior walls, outside, ragged tiles, and cell
    counts that split a tile over several workgroups."""
    T, B, ld = ROWS["T"], ROWS["B"], ROWS["pos_ld"]
    out = []
    for ri, rn in enumerate(ROOMS):
        r = room(rn)
        for ti, tn in enumerate(TABLES):
            rs = np.random.RandomState([73, ri, ti])
            out.append((f"inside-{rn}-{tn}", dict(room=rn, table=tn, pos=_layout(r["inside"](rs, T * B), T, B), pos_ld=ld,
                                                  n=8, cap=0.0, inside=True)))
    # the four on-edge positions as a tile of their own — the third of a launch whose first two tiles are interior (they
    # stay on the fast path and give the case the pairs its cap is a share of: the rays that run ALONG the edge a position
    # stands on, two or three per position, are decisions at a corner and are left out) — and one on-edge position among
    # 63 interior ones (positions 64 .. 127 of the launch: the second tile)
    for ri, rn in enumerate(("box", "maze", "box_polygon", "comb64", "interior_first")):
        rs = np.random.RandomState([77, ri])
        pos = np.concatenate((room(rn)["inside"](rs, 128), EDGE_POSITIONS))
        for tn in ("K180", "K51", "K360", "K180moved", "K16scrambled"):
            out.append((f"edges-{rn}-{tn}", dict(room=rn, table=tn, pos=_layout(pos, 1, 132), pos_ld=136, n=8, cap=CAP,
                                                 inside=False, edge_tile=128)))
    for e in range(4):
        rs = np.random.RandomState([79, e])
        pos = room("maze")["inside"](rs, T * B)
        pos[64 + 17 * e + 5] = EDGE_POSITIONS[e]
        out.append((f"edge-lane-{e}-maze-K180", dict(room="maze", table="K180", pos=_layout(pos, T, B), pos_ld=ld, n=8,
                                                     cap=CAP, inside=False, edge_lane=64 + 17 * e + 5)))
    # on interior walls, at their free ends, and outside the room
    for ri, rn in enumerate(ROOMS):
        for tn in ("K180", "K51", "K16scrambled"):
            rs = np.random.RandomState([83, ri])
            out.append((f"mixed-{rn}-{tn}", dict(room=rn, table=tn, pos=_layout(_mixed(room(rn), rs, T * B), T, B), pos_ld=ld,
                                                 n=8, cap=CAP, inside=False)))
    # ragged last tiles
    for P in (65, 1):
        for tn in ("K180", "K51"):
            rs = np.random.RandomState([89, P])
            out.append((f"ragged-P{P}-{tn}", dict(room="maze", table=tn, pos=_layout(room("maze")["inside"](rs, P), 1, P),
                                                  pos_ld=P + 3, n=8, cap=0.0, inside=True)))
    # several workgroups per tile: only part 0 writes ray_out
    for n, split in SPLITS:
        rs = np.random.RandomState([97, n])
        for rn in ("maze", "maze_polygon"):
            out.append((f"split{split}-n{n}-{rn}", dict(room=rn, table="K180", pos=_layout(room(rn)["inside"](rs, T * B), T, B),
                                                        pos_ld=ld, n=n, cap=0.0, inside=True, split=split)))
    rs = np.random.RandomState(101)
    out.append(("split2-n253-129tiles", dict(room="maze", table="K180", pos=_layout(room("maze")["inside"](rs, 8256), 3, 2752),
                                             pos_ld=2752, n=253, cap=0.0, inside=True, split=2)))
    return out


SPLITS = ((60, 1), (61, 2), (125, 4), (253, 8))
STAGE_B_COUNTS = (1, 5, 60, 61, 125, 253)     # a ragged last group, and every split


# ----------------------------------------------------------------------------- device tables
def ray_rden(walls, dirs):
    """BoundaryVectorCells._call: the position-independent denominators sa . sb_p of utils.vector_intercepts."""
    walls = np.asarray(walls, dtype=np.float64).reshape(-1, 2, 2)
    s_w = walls[:, 1, :] - walls[:, 0, :]
    with np.errstate(divide="ignore"):
        return 1.0 / (dirs[:, None, 0] * (-s_w[None, :, 1]) + dirs[:, None, 1] * s_w[None, :, 0])


def bvc_tables(walls, angles, dirs, mu_d, sg_d, mu_t, sg_t, ego):
    """The tables of `riab_boundary_vector_cells` with the expressions of BoundaryVectorCells._call (no direction
    windows): dict(test_dirs, ray_rden float64; cells (4, n), vm (n, Kp) | (2, n, Kp), inv_norm (n) float32; K)."""
    mu_d, sg_d, mu_t, sg_t = (np.asarray(v, dtype=np.float64) for v in (mu_d, sg_d, mu_t, sg_t))
    n, K = len(mu_d), len(angles)
    a = np.sqrt(LOG2E / 2) / sg_d
    kappa = 1 / sg_t ** 2
    cells = np.zeros((4, n))
    cells[0], cells[1], cells[2] = a * mu_d, a, kappa * LOG2E
    diff = angles[None, :] - mu_t[:, None]
    Kp = kernel_kp(K)
    if ego:
        vm = np.zeros((2, n, Kp))
        vm[0, :, :K], vm[1, :, :K] = np.cos(diff), np.sin(diff)
    else:
        vm = np.full((n, Kp), -np.inf)
        vm[:, :K] = LOG2E * kappa[:, None] * (np.cos(diff) - 1)
    norm = np.exp(kappa.reshape(-1, 1) * (np.cos(angles.reshape(1, -1)) - 1)).sum(axis=1)
    return dict(test_dirs=np.ascontiguousarray(dirs, dtype=np.float64), ray_rden=np.ascontiguousarray(ray_rden(walls, dirs)),
                cells=cells.astype(np.float32), vm=vm.astype(np.float32), inv_norm=(1 / norm).astype(np.float32), K=K)


# ----------------------------------------------------------------------------- the oracle, with its choice
def oracle_rays(pos, walls, dirs):
    """oracle.bvc_ray_distances restated with the wall it chose: (ref (P, K), first (P, K), l_a, l_b (P, K, W))."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    P, K = len(pos), len(dirs)
    segs = np.empty((P, K, 2, 2))
    segs[:, :, 0, :] = pos[:, None, :]
    segs[:, :, 1, :] = pos[:, None, :] + dirs[None, :, :]
    l_a, l_b = orc.segment_intercepts(segs.reshape(-1, 2, 2), walls)
    l_a, l_b = l_a.reshape(P, K, -1), l_b.reshape(P, K, -1)
    pref = np.zeros_like(l_a)
    with np.errstate(divide="ignore", invalid="ignore"):
        pref = np.where(l_a > 0, 1 / l_a, pref)
    pref = np.where(l_a < 0, -1.0, pref)
    pref = np.where(l_b < 0, -1.0, pref)
    pref = np.where(l_b > 1, -1.0, pref)
    first = np.argmax(pref, axis=-1)
    return np.take_along_axis(l_a, first[..., None], axis=-1)[..., 0], first, l_a, l_b


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def ray_tolerance(pos, walls, dirs, ref, first):
    """One float32 ulp of the reference + the cancellation bound of the chosen wall's numerator,
    4 eps64 (|d0x sy| + |d0y sx|) |rden| — from the inputs alone (the device may or may not contract the numerator)."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    walls = np.asarray(walls, dtype=np.float64).reshape(-1, 2, 2)
    s = walls[:, 1, :] - walls[:, 0, :]
    d0 = walls[None, :, 0, :] - pos[:, None, :]                           # (P, W, 2)
    mag = np.abs(d0[..., 0] * s[None, :, 1]) + np.abs(d0[..., 1] * s[None, :, 0])   # (P, W)
    rd = np.abs(ray_rden(walls, dirs))                                    # (K, W)
    P, K = first.shape
    cancel = 4 * EPS64 * mag[np.arange(P)[:, None], first] * rd[np.arange(K)[None, :], first]
    with np.errstate(invalid="ignore"):
        return ulp32(np.where(np.isfinite(ref), ref, 0.0)) + np.where(np.isfinite(cancel), cancel, 0.0)


def exclusions(ref, first, l_a, l_b):
    """(P, K) bool: the pairs that may be left out, and nothing else —
    1. the oracle's decision is within NEAR of flipping: l_b within NEAR of 0 or 1 on the chosen wall or on a wall whose
       crossing lies ahead and no farther than the chosen one (every wall ahead, for a miss), or a wall with its crossing on
       the segment whose l_a is within NEAR of 0 without being 0 (the exact zeros of a position ON a wall are compared);
    2. the oracle's value is not finite;
    3. a miss (the wall-0 fallback) with |ref| > FALLBACK_BIG."""
    with np.errstate(invalid="ignore"):
        chosen_b = np.take_along_axis(l_b, first[..., None], axis=-1)[..., 0]
        hit = (ref > 0) & ~(chosen_b < 0) & ~(chosen_b > 1)
        zero = (ref == 0) & ~(chosen_b < 0) & ~(chosen_b > 1)                # standing on the chosen wall
        reach = np.where(hit, ref, np.inf)[..., None]
        b_edge = (np.abs(l_b) <= NEAR) | (np.abs(l_b - 1) <= NEAR)
        ahead = (l_a > 0) & (l_a <= reach * (1 + NEAR) + NEAR)
        near_b = (b_edge & ahead & ~zero[..., None]).any(axis=-1)
        on_seg = (l_b >= -NEAR) & (l_b <= 1 + NEAR)
        near_a = ((np.abs(l_a) <= NEAR) & (l_a != 0) & on_seg).any(axis=-1)
        # (standing on a wall: the zero wins only while no wall ahead is hit, so the walls ahead are the decision)
        near_zero = zero & (b_edge & (l_a > 0)).any(axis=-1)
        chosen_edge = np.take_along_axis(b_edge, first[..., None], axis=-1)[..., 0]
        miss = ~hit & ~zero
        big = miss & (np.abs(ref) > FALLBACK_BIG)
    return near_b | near_a | near_zero | chosen_edge | ~np.isfinite(ref) | big


# ----------------------------------------------------------------------------- stage A restated
def kernel_rays(r, pos, dirs, fix=True):
    """Stage A of bvc_kernel in NumPy float64 -> float32 (P, K): the same `rden` table, `num * rden` instead of the
    reference's division, the box fast path per tile, a ray and its opposite from one pair of intercepts where the table is
    paired, `valid`, `best` and the wall-0 fallback — and (`fix`) the second look of a miss for a wall the position
    stands on.  `fix=False` is the kernel before that look."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    walls = np.asarray(r["walls"], dtype=np.float64).reshape(-1, 2, 2)
    K, P = len(dirs), len(pos)
    rden = ray_rden(walls, dirs)
    s = walls[:, 1, :] - walls[:, 0, :]
    d0 = walls[None, :, 0, :] - pos[:, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        num = d0[..., 0] * (-s[None, :, 1]) + d0[..., 1] * s[None, :, 0]                       # (P, W)
        la = num[:, None, :] * rden[None]                                                      # (P, K, W)
        lb = ((-d0[:, None, :, 0]) * (-dirs[None, :, None, 1]) + (-d0[:, None, :, 1]) * dirs[None, :, None, 0]) * (-rden[None])
        on_seg = ~(lb < 0) & ~(lb > 1)
        box = np.repeat(kernel_box4(r, pos), 64)[:P]
        on_hot = on_seg.copy()
        on_hot[box, :, :4] = True                                                              # the edges' l_b is not computed
        src = np.arange(K)
        sign = np.ones(K)
        if kernel_paired(dirs):
            m = K >> 1
            n_pairs = K - 1 - m
            src[1 + m:1 + m + n_pairs] = np.arange(1, n_pairs + 1)
            sign[1 + m:1 + m + n_pairs] = -1.0
        la_k = sign[None, :, None] * la[:, src, :]
        best = np.where(on_hot[:, src, :] & (la_k > 0), la_k, np.inf).min(axis=-1)
        d = np.where(best < np.inf, best, la_k[:, :, 0])
        if fix:
            stands = ((la[:, src, :] == 0) & on_seg[:, src, :]).any(axis=-1)
            d = np.where(~(best < np.inf) & stands, 0.0, d)
        return d.astype(np.float32)


# ----------------------------------------------------------------------------- stage B
def stage_b_cells(n, seed=103):
    """n cells with the reference's default spread of tunings (Neurons.py:1478-1530, "random"), from a fixed seed."""
    rs = np.random.RandomState([seed, n])
    mu_d = rs.uniform(0.0, 0.3, n)
    mu_t = rs.uniform(0, 2 * np.pi, n)
    sg_t = np.radians(rs.uniform(8, 30, n))
    sg_d = mu_d / 12 + 0.08
    return mu_d, sg_d, mu_t, sg_t


# Rooms of the class tests (positions on the room's edges, compared through rates under the project's own check): the open
# box, and a room whose interior walls touch no edge.  The maze is NOT among them: its walls end ON the edges — (0.4, 1),
# (0.8, 1), (0.2, 0), (0.6, 0) — so the ray that runs along the edge from an on-edge position grazes a wall's end, and the
# oracle, which builds that ray as (pos + u) - pos, and the kernel, which takes the table's (-1, 1.2e-16) as it is, decide
# the graze at l_b = -+3e-17 either way (0.5 against 0.1 from (0.5, 1)): a decision within 1e-9 of flipping, which the ray
# tests leave out pair by pair and a rate cannot (tests/test_bvc_rays_cpu.py asserts both statements).
CLASS_WALLS = ((), ([[.3, .5], [.7, .5]], [[.25, .2], [.25, .4]]))


def class_positions():
    """The four on-edge positions and 60 interior ones, with head directions."""
    rs = np.random.RandomState(109)
    pos = np.concatenate((EDGE_POSITIONS, f32(rs.uniform(0.01, 0.99, (60, 2)))))
    a = rs.uniform(0, 2 * np.pi, len(pos))
    return pos, f32(np.stack((np.cos(a), np.sin(a)), axis=-1))


def tune(cells, mu):
    """Give a BoundaryVectorCells population the tunings `mu` = (mu_d, sg_d, mu_t, sg_t) — and the normalisation that goes
    with them, which the class (like the reference) computes from sigma_angles once, in __init__."""
    cells.tuning_distances, cells.sigma_distances, cells.tuning_angles, cells.sigma_angles = (np.array(v) for v in mu)
    kappa = 1 / np.asarray(cells.sigma_angles, dtype=float).reshape(-1, 1) ** 2
    cells.cell_fr_norm = np.exp(kappa * (np.cos(cells.test_angles.reshape(1, -1)) - 1)).sum(axis=1)
    return cells


def stage_b_reference(d, angles, mu_d, sg_d, mu_t, sg_t, hd=None, keep=None):
    """The float64 sum oracle.bvc forms, over the distances `d` (P, K) given -> (n, P).  `keep` (n, K) bool: the terms a
    direction window keeps (None: all)."""
    th = np.broadcast_to(angles[None, :], d.shape)
    if hd is not None:
        th = th - orc.get_angle(np.asarray(hd, dtype=np.float64).reshape(-1, 2))[:, None]
    g = orc.gaussian(d[None], mu_d[:, None, None], sg_d[:, None, None]) * orc.von_mises(th[None], mu_t[:, None, None], sg_t[:, None, None])
    if keep is not None:
        g = g * keep[:, None, :]
    return g.sum(axis=-1) / orc.bvc_fr_norm(angles, sg_t)[:, None]


def stage_b_float32(d, tabs, hd=None):
    """The same sum as stage B writes it, in NumPy float32 with plain operations (no FMA, NumPy's exp2; not the device):
    exp2(-(a d - a mu)^2 + T[c][k]) summed over k in order, times inv_norm -> (n, P) float32."""
    f = np.float32
    d = np.asarray(d, dtype=f)
    cells, vm, inv = tabs["cells"], tabs["vm"], tabs["inv_norm"]
    K = tabs["K"]
    tt = d[None] * cells[1][:, None, None] - cells[0][:, None, None]              # (n, P, K)
    if hd is None:
        v = vm[:, None, :K]
    else:
        h = np.asarray(hd, dtype=f).reshape(-1, 2)
        hx, hy = h[:, 0] + f(1e-6), h[:, 1]
        inv_h = f(1) / np.sqrt(hx * hx + hy * hy)
        ch, sh = hx * inv_h, hy * inv_h
        rot = vm[0][:, None, :K] * ch[None, :, None] + vm[1][:, None, :K] * sh[None, :, None]
        v = cells[2][:, None, None] * (rot - f(1))
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp2((-tt * tt + v).astype(f))
    acc = np.zeros(e.shape[:2], dtype=f)
    for k in range(K):
        acc = acc + e[:, :, k]
    return (acc * inv[:, None]).astype(f)
