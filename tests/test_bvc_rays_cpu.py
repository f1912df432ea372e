"""What tests/bvc_ray_cases.py claims about its own cases, checked with the oracle alone (no GPU), so that
tests/test_gpu_bvc_rays.py cannot pass vacuously: every table and room reaches the branch of `bvc_kernel`'s stage A it is
named after (by the kernel's own `paired`, four-edge, `split` and Kp rules, restated), the table helper builds what
`BoundaryVectorCells._call` builds, the pairs left out of the ray comparison stay under their caps (a property of the
inputs, not of the kernel), and a NumPy restatement of stage A meets the GPU test's bound everywhere else — after the
on-edge fix; before it, it disagrees with the oracle on the on-edge positions, on exactly the rays that leave the room."""
import ctypes as C

import numpy as np
import pytest

from oracle import riab_oracle as orc
from tests import bvc_ray_cases as bc

CASES = bc.ray_cases()


def _f32_exact(a):
    return np.array_equal(a, a.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("name", list(bc.TABLES))
def test_tables_reach_the_branches_they_name(name):
    _build, K, paired, _what = bc.TABLES[name]
    angles, dirs = bc.table(name)
    assert dirs.shape == (K, 2) and angles.shape == (K,)
    np.testing.assert_allclose(np.linalg.norm(dirs, axis=1), 1.0, atol=2e-9)
    np.testing.assert_allclose(dirs, np.stack((np.cos(angles), np.sin(angles)), axis=-1), atol=2e-9)
    assert bc.kernel_paired(dirs) == paired
    m, n_pairs = K >> 1, K - 1 - (K >> 1)
    if name == "K180":
        assert n_pairs == 89 and 1 + (m - n_pairs) == 2                  # cast_single(2, 89): table indices 0 and 90
    if name == "K51":
        assert K % 2 == 1 and bc.kernel_kp(K) == 52 and K % 32 != 0      # a pad row; 8 waves x 4 rays: the last batch is clamped
    if name == "K12":
        assert K % 2 == 0 and n_pairs == 5 and np.abs(dirs[1:6] + dirs[7:12]).max() <= 1e-12   # opposites, but too few pairs
    if name == "K18":
        assert n_pairs == 8
    if name == "K360":
        assert 64 * 1024 < bc.kernel_kp(K) * 64 * 4 <= 160 * 1024
    if name == "K7":
        assert K % 4 != 0 and bc.kernel_kp(K) == 8
    if name == "K180moved":
        ref = bc.table("K180")[1]
        assert (dirs != ref).sum() == 1 and 1e-12 < np.abs(dirs - ref).max() <= 1.0000001e-9
    if name == "K16scrambled":
        for axis in ([1, 0], [0, 1], [-1, 0], [0, -1]):
            assert (dirs == np.array(axis, dtype=float)).all(axis=1).sum() == 1
        assert not np.array_equal(np.argsort(angles), np.arange(K))


@pytest.mark.parametrize("name", list(bc.ROOMS))
def test_rooms_take_the_paths_they_name(name):
    edges_ok, _what = bc.ROOMS[name]
    r = bc.room(name)
    walls = np.asarray(r["walls"])
    assert bc.kernel_box_edges(r) == edges_ok
    assert 4 <= len(walls) <= 64
    pos = r["inside"](np.random.RandomState(1), 300)
    assert len(pos) == 300 and _f32_exact(pos)
    assert bc.kernel_box4(r, pos).all() == edges_ok
    if name.endswith("_polygon"):
        assert np.array_equal(walls, bc.room(name[:-len("_polygon")])["walls"]) and r["polygon"] == 1
    if name == "comb64":
        from ratinabox_amd import _lib
        assert len(walls) == 64 == _lib.MAX_WALLS
    if name == "lroom":
        a, b = walls[0]
        assert r["polygon"] == 1 and a[1] == b[1] == 0.5 and list(r["extent"]) == [0, 1, 0, 1]   # the notch: on no edge of the extent
        assert orc.polygon_contains(np.asarray(bc.L_ROOM, dtype=float), pos).all()
    if name == "interior_first":
        maze = bc.room("maze")["walls"]
        assert r["polygon"] == 0 and len(walls) == 9
        assert sorted(map(tuple, walls.reshape(-1, 4))) == sorted(map(tuple, maze.reshape(-1, 4)))
        assert np.array_equal(walls[:2], maze[4:6]) and np.array_equal(walls[2:6], maze[:4])
    if len(r["on_walls"]):
        # "on an interior wall": within a float32 rounding of a wall that is not one of the room's first four edges
        d = np.linalg.norm(orc.shortest_vectors_from_walls(r["on_walls"], walls), axis=-1)
        interior = np.ones(len(walls), dtype=bool)
        interior[[i for i, w in enumerate(walls) if any(np.array_equal(w, e) for e in orc.EnvSpec().walls)]] = False
        assert (d[:, interior].min(axis=1) <= 3e-8).all()
        ends = np.linalg.norm(r["on_walls"][:, None, None, :] - walls[None, interior], axis=-1).min(axis=(1, 2))
        assert (ends <= 3e-8).sum() >= 2 and (ends > 0.01).sum() >= 2       # free ends and mid-wall positions


def test_cases_reach_the_tiles_and_splits_they_name():
    ids = [cid for cid, _ in CASES]
    assert len(set(ids)) == len(ids)
    seen_splits = set()
    for cid, c in CASES:
        r = bc.room(c["room"])
        T, B, _ = c["pos"].shape
        pos = c["pos"].reshape(-1, 2)
        assert _f32_exact(pos) and np.isfinite(pos).all(), cid
        assert T * B <= 320 or cid == "split2-n253-129tiles", cid
        box = bc.kernel_box4(r, pos)
        e0, e1, e2, e3 = r["extent"]
        strictly = (pos[:, 0] > e0) & (pos[:, 0] < e1) & (pos[:, 1] > e2) & (pos[:, 1] < e3)
        if c["inside"]:
            assert strictly.all() and c["cap"] == 0.0, cid
            assert box.all() == bc.ROOMS[c["room"]][0], cid
        else:
            assert c["cap"] == bc.CAP and not strictly.all(), cid
        if cid.startswith("inside-"):
            assert (T, B, c["pos_ld"]) == (3, 68, 72) and len(box) == 4 and B % 64 != 0 and c["pos_ld"] != B
        if "edge_tile" in c:
            # a tile of their own: the four on-edge positions are the only live lanes of the last tile
            assert c["edge_tile"] % 64 == 0 and np.array_equal(pos[c["edge_tile"]:], bc.EDGE_POSITIONS)
            assert strictly[:c["edge_tile"]].all() and not strictly[c["edge_tile"]:].any()
            assert not box[-1] and box[:-1].all() == bc.ROOMS[c["room"]][0], cid
        if "edge_lane" in c:
            # one on-edge lane among 63 interior ones: the whole tile leaves the fast path, the others stay on it
            lane = c["edge_lane"]
            assert (~strictly).sum() == 1 and not strictly[lane] and 64 <= lane < 128
            assert list(box) == [True, False, True, True], cid
        if cid.startswith("mixed-"):
            assert list(np.nonzero(~strictly)[0] // 64) == [1, 1], cid           # the two outside positions, in tile 1
            if bc.ROOMS[c["room"]][0]:
                assert list(box) == [True, False, True, True], cid
        if cid.startswith("ragged-"):
            assert T * B in (65, 1)
        assert bc.kernel_split(c["n"], T * B) == c.get("split", 1), cid
        seen_splits.add((c["n"], bc.kernel_split(c["n"], T * B), (T * B + 63) // 64))
    assert {(60, 1, 4), (61, 2, 4), (125, 4, 4), (253, 8, 4), (253, 2, 129)} <= seen_splits
    assert 129 * 2 * 2 > 512 >= 129 * 1 * 2                                      # what holds the large case at split 2
    # every table in every room
    assert {(c["room"], c["table"]) for _, c in CASES} >= {(r, t) for r in bc.ROOMS for t in bc.TABLES}


@pytest.mark.parametrize("group", ["inside", "edges", "edge-lane", "mixed", "ragged", "split"])
def test_exclusions_stay_under_their_caps_and_the_restatement_meets_the_bound(group):
    """Per case: the oracle with its choice IS the oracle; the pairs left out are at most 0.5 % of the case (none for
    positions strictly inside); everywhere else the kernel's stage A restated in float64 NumPy is within the GPU test's
    bound of the oracle rounded to float32; and the on-edge positions keep the rays the fix is about."""
    cases = [(cid, c) for cid, c in CASES if cid.startswith(group)]
    assert cases
    total = left_out = 0
    for cid, c in cases:
        r = bc.room(c["room"])
        _angles, dirs = bc.table(c["table"])
        pos = c["pos"].reshape(-1, 2)
        ref, first, l_a, l_b = bc.oracle_rays(pos, r["walls"], dirs)
        if len(pos) <= 320:
            assert np.array_equal(ref, orc.bvc_ray_distances(pos, r["walls"], dirs), equal_nan=True), cid
        ex = bc.exclusions(ref, first, l_a, l_b)
        assert ex.sum() <= int(c["cap"] * ex.size), (cid, int(ex.sum()), ex.size)
        tol = bc.ray_tolerance(pos, r["walls"], dirs, ref, first)
        got = bc.kernel_rays(r, pos, dirs).astype(np.float64)
        with np.errstate(invalid="ignore"):
            bad = (np.abs(got - ref.astype(np.float32).astype(np.float64)) > tol) & ~ex
        assert not bad.any(), (cid, int(bad.sum()))
        assert (tol[~ex] < 1e-6 * np.maximum(np.abs(ref[~ex]), 1e-30) + 1e-44).all(), cid   # the bound is a few float32 ulps, nothing wider
        total += ex.size
        left_out += int(ex.sum())
        if "edge_tile" in c or "edge_lane" in c:
            lanes = range(c["edge_tile"], len(pos)) if "edge_tile" in c else [c["edge_lane"]]
            K = len(dirs)
            for p in lanes:
                zeros = (ref[p] == 0) & ~ex[p]
                assert zeros.sum() >= K // 2 - 4, (cid, p, int(zeros.sum()))         # the rays that leave the room: compared, and 0
                assert ex[p].sum() <= 4, (cid, p)                                    # only the rays along the edge are left out
    print(f"bvc-rays {group}: {left_out} of {total} pairs left out")


def test_stage_a_before_and_after_the_fix_on_the_edges():
    """The default box in the project's own wall order, the reference table: before the fix the kernel's form disagrees
    with the oracle on 89 of 180 rays at (0, 0.5), (1, 0.25) and (0.5, 1) — the rays that leave the room, which the
    oracle reads as 0 — and on none at (0.5, 0), where wall 0 is the edge itself and its l_a is the fallback; after the
    fix on none anywhere.  A cell tuned 6 cm behind such a position: 0.78 in the reference, ~0 before the fix."""
    r = bc.room("box")
    angles, dirs = bc.table("K180")
    pos = bc.EDGE_POSITIONS
    ref, first, l_a, l_b = bc.oracle_rays(pos, r["walls"], dirs)
    ex = bc.exclusions(ref, first, l_a, l_b)
    tol = bc.ray_tolerance(pos, r["walls"], dirs, ref, first)
    ref32 = ref.astype(np.float32).astype(np.float64)
    before, after = (bc.kernel_rays(r, pos, dirs, fix=f).astype(np.float64) for f in (False, True))
    with np.errstate(invalid="ignore"):
        differs = ~(np.abs(before - ref32) <= tol)
        assert not (~(np.abs(after - ref32) <= tol) & ~ex).any()
    assert differs.sum(axis=1).tolist() == [89, 89, 0, 89]
    outward = np.array([dirs[:, 0] < -1e-9, dirs[:, 0] > 1e-9, dirs[:, 1] < -1e-9, dirs[:, 1] > 1e-9])
    for p in (0, 1, 3):
        assert np.array_equal(differs[p], outward[p]) and (ref[p][outward[p]] == 0).all() and not ex[p][outward[p]].any()
        assert not np.isfinite(before[p][outward[p]]).all() or np.abs(before[p][outward[p]]).max() > 1e3 or before[p][outward[p]].min() < 0
    # the rate of a cell tuned to a wall 6 cm behind (0, 0.5): sigma_d = mu_d / 12 + 0.08 (the reference's), 11.25 degrees
    mu_d, sg_d, mu_t, sg_t = np.array([0.06]), np.array([0.06 / 12 + 0.08]), np.array([np.pi]), np.array([np.radians(11.25)])
    want = bc.stage_b_reference(ref[:1], angles, mu_d, sg_d, mu_t, sg_t)
    np.testing.assert_allclose(want, orc.bvc(pos[:1], r["walls"], mu_d, mu_t, sg_d, sg_t), rtol=1e-13)
    was = bc.stage_b_reference(before[:1], angles, mu_d, sg_d, mu_t, sg_t)
    now = bc.stage_b_reference(after[:1], angles, mu_d, sg_d, mu_t, sg_t)
    assert want[0, 0] > 0.7 and was[0, 0] < 0.01 and abs(now[0, 0] - want[0, 0]) < 1e-7, (want, was, now)


@pytest.mark.parametrize("ego", [False, True], ids=["allo", "ego"])
def test_table_helper_builds_what_the_class_builds(ego, monkeypatch):
    import ratinabox_amd as riab
    np.random.seed(5)
    env = riab.Environment({"walls": bc.MAZE})
    ag = riab.Agent(env, {"device": "cpu"})
    B = riab.BoundaryVectorCells(ag, {"n": 13, "reference_frame": "egocentric" if ego else "allocentric"})
    assert np.array_equal(np.asarray(env.walls), bc.room("maze")["walls"])
    angles, dirs = bc.table("K180")
    assert np.array_equal(angles, B.test_angles) and np.array_equal(dirs, B.test_directions)
    mine = bc.bvc_tables(env.walls, angles, dirs, B.tuning_distances, B.sigma_distances, B.tuning_angles, B.sigma_angles, ego)
    monkeypatch.setenv("RIAB_NO_BVC_WINDOWS", "1")
    d = B._call(None, None)
    assert "cell_rows" not in d and d["K"] == 180 and d["egocentric"] == int(ego)
    for key, theirs in (("test_dirs", "test_dirs"), ("ray_rden", "ray_rden"), ("cells", "table"), ("vm", "vm_table"),
                        ("inv_norm", "inv_norm")):
        got = d[theirs].numpy()
        assert got.dtype == mine[key].dtype and np.array_equal(got, mine[key], equal_nan=True), key
    if not ego:
        # with direction windows the class hands the same rows over in another order
        monkeypatch.delenv("RIAB_NO_BVC_WINDOWS")
        B._table_cache.clear()
        d = B._call(None, None)
        order = d["cell_rows"].numpy()
        assert sorted(order.tolist()) == list(range(13))
        assert np.array_equal(d["table"].numpy(), mine["cells"][:, order]) and np.array_equal(d["vm_table"].numpy(), mine["vm"][order])
        assert np.array_equal(d["inv_norm"].numpy(), mine["inv_norm"][order])
    # the other resolutions' tables are the reference's too
    for name, dtheta in (("K51", 7), ("K12", 30), ("K18", 20), ("K360", 1), ("K7", 51)):
        Bd = riab.BoundaryVectorCells(ag, {"n": 2, "dtheta": dtheta})
        assert np.array_equal(bc.table(name)[1], Bd.test_directions) and np.array_equal(bc.table(name)[0], Bd.test_angles)


def test_stage_b_restatement_is_the_oracle_sum():
    """`stage_b_reference` over the oracle's own distances is oracle.bvc; the float32 restatement is close to it (what sizes
    the stage-B tolerance on the device); the windowed tables of the cell counts the GPU test uses hold a window that wraps
    past K."""
    import ratinabox_amd as riab
    r = bc.room("maze")
    angles, dirs = bc.table("K180")
    rs = np.random.RandomState(3)
    pos = r["inside"](rs, 40)
    hd = bc.f32(np.stack((np.cos(np.arange(40.0)), np.sin(np.arange(40.0))), axis=-1))
    d = orc.bvc_ray_distances(pos, r["walls"], dirs)
    wraps = 0
    for n in bc.STAGE_B_COUNTS:
        mu_d, sg_d, mu_t, sg_t = bc.stage_b_cells(n)
        for h in (None, hd):
            want = bc.stage_b_reference(d, angles, mu_d, sg_d, mu_t, sg_t, hd=h)
            np.testing.assert_allclose(want, orc.bvc(pos, r["walls"], mu_d, mu_t, sg_d, sg_t, head_direction=h), rtol=1e-12, atol=1e-300)
            tabs = bc.bvc_tables(r["walls"], angles, dirs, mu_d, sg_d, mu_t, sg_t, h is not None)
            got = bc.stage_b_float32(d, tabs, hd=h)
            assert got.dtype == np.float32 and 0 < np.abs(got - want).max() < 1e-5, (n, np.abs(got - want).max())
        ag = riab.Agent(riab.Environment({"walls": bc.MAZE}), {"device": "cpu"})
        B = riab.BoundaryVectorCells(ag, {"n": n})
        bc.tune(B, (mu_d, sg_d, mu_t, sg_t))
        t = B._call(None, None)
        mine = bc.bvc_tables(r["walls"], angles, dirs, mu_d, sg_d, mu_t, sg_t, False)
        order = t["cell_rows"].numpy() if "cell_rows" in t else np.arange(n)
        # the class's tables for these cells are the helper's rows in the class's order — the normalisation included
        assert np.array_equal(t["inv_norm"].numpy(), mine["inv_norm"][order]), n
        assert np.array_equal(t["table"].numpy(), mine["cells"][:, order]) and np.array_equal(t["vm_table"].numpy(), mine["vm"][order])
        if "windows" in t:
            win = t["windows"].numpy()
            assert (win % 4 == 0).all() and (win[:, 1] > 0).all() and (win[:, 1] <= 180).all()
            wraps += int((win.sum(axis=1) > 180).sum())
    assert wraps >= 1


def test_class_test_rooms_hold_no_knife_edge_but_the_maze_does():
    """The rooms of the class tests: at the on-edge positions the oracle leaves out only rays along the edge stood on, and
    on those the kernel's form agrees anyway (corner hits with exact l_b), so rates from the restated stage A meet the
    project's check against oracle.bvc.  In the maze the ray along the top edge from (0.5, 1) grazes the end of the wall at
    (0.4, 1): the oracle's l_b there is -3e-17 (a miss: 0.5, the far corner), the kernel's form with the table's own direction hits the end (0.1) — why the maze is not used there."""
    angles, dirs = bc.table("K180")
    pos, _hd = bc.class_positions()
    mu_d, sg_d, mu_t, sg_t = bc.stage_b_cells(40)
    for walls in bc.CLASS_WALLS:
        r = dict(bc.room("box"), walls=orc.EnvSpec(walls=walls).walls)
        ref, first, l_a, l_b = bc.oracle_rays(pos, r["walls"], dirs)
        ex = bc.exclusions(ref, first, l_a, l_b)
        got = bc.kernel_rays(r, pos, dirs).astype(np.float64)
        assert ex[4:].sum() == 0 and (ex[:4].sum(axis=1) <= 3).all()
        assert np.array_equal(got[ex], ref[ex])                                   # left out, and still the same
        want = orc.bvc(pos, r["walls"], mu_d, mu_t, sg_d, sg_t)
        mine = bc.stage_b_reference(got, angles, mu_d, sg_d, mu_t, sg_t)
        assert (np.abs(mine - want) <= 1e-5 * np.abs(want) + 1e-5).all() and (want[:, :4] > 0.01).any()
    r = bc.room("maze")
    ref, first, l_a, l_b = bc.oracle_rays(bc.EDGE_POSITIONS[3:], r["walls"], dirs)
    assert ref[0, 91] == 0.5 and bc.exclusions(ref, first, l_a, l_b)[0, 91]
    grazed = int(np.argmin(np.abs(l_a[0, 91] - 0.1)))
    assert np.array_equal(r["walls"][grazed][0], [0.4, 1.0]) and l_b[0, 91, grazed] < 0 and abs(l_b[0, 91, grazed]) <= 1e-15
    assert bc.kernel_rays(r, bc.EDGE_POSITIONS[3:], dirs)[0, 91] == np.float32(0.1)


def test_ray_out_with_windows_passes_the_argument_checks():
    """`ray_out` together with direction windows is an accepted combination: such a call gets past the checks of the
    window arguments and is refused only for a later reason (here: too many walls), before anything is launched; the same
    call with windows the kernel cannot take is refused for those."""
    from ratinabox_amd import _lib as L
    env, io = L.RiabEnv(), L.RiabRateIO()
    env.n_walls, env.walls = 1000, 64
    io.T, io.B, io.pos_ld = 1, 4, 4
    io.pos_x = io.pos_y = io.hd_x = io.hd_y = io.rates = 64          # never dereferenced: every call returns before a launch
    p = C.c_void_p(64)
    f = L.lib.riab_boundary_vector_cells_windowed
    assert f(env, io, p, p, 180, p, p, p, 8, 0, p, p, p, None) == L.ETOOBIG           # ray_out + rows + windows
    assert f(env, io, p, p, 180, p, p, p, 8, 0, None, p, p, None) == L.ETOOBIG
    assert f(env, io, p, p, 180, p, p, p, 8, 0, p, None, None, None) == L.ETOOBIG
    assert f(env, io, p, p, 180, p, p, p, 8, 0, p, p, None, None) == L.EINVAL         # rows without windows
    assert f(env, io, p, p, 180, p, p, p, 8, 1, p, p, p, None) == L.EUNSUPPORTED      # windows are allocentric
    assert f(env, io, p, p, 51, p, p, p, 8, 0, p, p, p, None) == L.EUNSUPPORTED       # ... and need K % 4 == 0
    assert L.lib.riab_boundary_vector_cells(env, io, p, p, 361, p, p, p, 8, 0, p, None) == L.ETOOBIG
