"""`bvc_kernel` (csrc/riab_bvc.hip) stage by stage, through `riab_boundary_vector_cells_windowed` with the ABI's `ray_out`
(tests/bvc_ray_cases.py builds the cases; tests/test_bvc_rays_cpu.py checks what they claim without a GPU):

1. stage A, ray by ray, against oracle.bvc_ray_distances: every element of `ray_out` [T][K][B] written, no bit of the guard
   behind it changed, |got - fp32(ref)| <= one fp32 ulp of ref + 4 eps64 (|d0x sy| + |d0y sx|) |rden| of the chosen wall;
   the pairs left out (decisions within 1e-9 of flipping, non-finite reference values, misses beyond 1e3) are at most
   0.5 % of a case and none for positions strictly inside the room;
2. stage B from the kernel's own rays: the float64 sum oracle.bvc forms over those float32 distances, under four times the
   error of a float32 NumPy restatement of the same sum (+ BVC_WINDOW_SHARE with direction windows);
3. the classes a user reaches, at positions on the room's edges, against oracle.bvc under the project's own check.

Every worst figure is printed (docs/EXPERIMENTS.md records them)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import riab_oracle as orc
from tests import bvc_ray_cases as bc

pytestmark = pytest.mark.gpu

RTOL = 1e-5
POISON = 0x7FC12345          # a NaN no arithmetic produces: what an element nobody wrote still holds
GUARD = 4096                 # elements behind each output
CASES = dict(bc.ray_cases())


@pytest.fixture(scope="module")
def riab():
    assert torch.cuda.is_available(), "these tests need the GPU"
    import ratinabox_amd
    return ratinabox_amd


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _rows(a, pos_ld):
    """(T, B) -> float32 [T][pos_ld] on the device, the columns past B holding a value no room contains."""
    T, B = a.shape
    t = torch.full((T, pos_ld), 1e30, dtype=torch.float32)
    t[:, :B] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.cuda()


def launch(riab, r, tabs, pos, pos_ld, hd=None, rows=None, win=None):
    """One call of riab_boundary_vector_cells_windowed with a RiabEnv / RiabRateIO of the test's own.  `tabs`: device
    tensors or NumPy arrays (test_dirs, ray_rden, cells, vm, inv_norm, K).  -> (rays (T, K, B), rates (T, n, B)) float32,
    after checking that every element of both was written and no bit of their guards changed."""
    L = riab._lib
    T, B, _ = pos.shape
    K, ego = int(tabs["K"]), hd is not None
    dev = {k: (v if torch.is_tensor(v) else _dev(v, np.float64 if k in ("test_dirs", "ray_rden") else np.float32))
           for k, v in tabs.items() if k != "K"}
    n = int(dev["cells"].shape[1])
    assert tuple(dev["test_dirs"].shape) == (K, 2) and tuple(dev["ray_rden"].shape) == (K, len(r["walls"]))
    assert tuple(dev["vm"].shape) == ((2, n, bc.kernel_kp(K)) if ego else (n, bc.kernel_kp(K))) and tuple(dev["inv_norm"].shape) == (n,)
    walls = _dev(np.asarray(r["walls"]).reshape(-1, 4), np.float64)
    env = L.RiabEnv()
    for i in range(4):
        env.extent[i] = float(r["extent"][i])
    env.scale, env.periodic, env.n_walls, env.walls = 1.0, 0, int(len(walls)), walls.data_ptr()
    env.polygon, env.n_boundary, env.hole_mask = int(r["polygon"]), int(r["n_boundary"]), 0
    px, py = _rows(pos[..., 0], pos_ld), _rows(pos[..., 1], pos_ld)
    io = L.RiabRateIO()
    io.pos_x, io.pos_y, io.pos_ld, io.T, io.B = px.data_ptr(), py.data_ptr(), pos_ld, T, B
    if ego:
        hx, hy = _rows(hd[..., 0], pos_ld), _rows(hd[..., 1], pos_ld)
        io.hd_x, io.hd_y = hx.data_ptr(), hy.data_ptr()
    rays = torch.full((T * K * B + GUARD,), POISON, dtype=torch.int32, device="cuda")
    rates = torch.full((T * n * B + GUARD,), POISON, dtype=torch.int32, device="cuda")
    io.rates, io.dt, io.min_fr, io.max_fr = rates.data_ptr(), 0.05, 0.0, 1.0
    rc = L.lib.riab_boundary_vector_cells_windowed(env, io, L.ptr(dev["test_dirs"]), L.ptr(dev["ray_rden"]), K, L.ptr(dev["cells"]),
                                                   L.ptr(dev["vm"]), L.ptr(dev["inv_norm"]), n, int(ego), C.c_void_p(rays.data_ptr()),
                                                   L.ptr(rows), L.ptr(win), L.current_stream())
    assert rc == 0, L.strerror(rc)
    torch.cuda.synchronize()
    out = []
    for buf, rows_ in ((rays, K), (rates, n)):
        bits = buf.cpu().numpy()
        assert (bits[T * rows_ * B:] == POISON).all(), "the guard behind an output changed"
        assert (bits[:T * rows_ * B] != POISON).all(), f"{int((bits[:T * rows_ * B] == POISON).sum())} elements were never written"
        out.append(bits[:T * rows_ * B].view(np.float32).reshape(T, rows_, B))
    return out[0], out[1]


_reference = {}


def reference(cid):
    """(ref, first, left out, bound) of a case, computed once."""
    if cid not in _reference:
        c = CASES[cid]
        r, (_angles, dirs), pos = bc.room(c["room"]), bc.table(c["table"]), c["pos"].reshape(-1, 2)
        ref, first, l_a, l_b = bc.oracle_rays(pos, r["walls"], dirs)
        _reference[cid] = (ref, first, bc.exclusions(ref, first, l_a, l_b), bc.ray_tolerance(pos, r["walls"], dirs, ref, first))
    return _reference[cid]


def default_cells(n, ego, angles, dirs, walls):
    mu_d, sg_d, mu_t, sg_t = bc.stage_b_cells(n)
    return bc.bvc_tables(walls, angles, dirs, mu_d, sg_d, mu_t, sg_t, ego)


# ----------------------------------------------------------------------------- 1. stage A
@pytest.mark.parametrize("cid", list(CASES))
def test_ray_distances_vs_oracle(riab, cid):
    c = CASES[cid]
    r, (angles, dirs) = bc.room(c["room"]), bc.table(c["table"])
    T, B, _ = c["pos"].shape
    K = len(dirs)
    ref, first, left_out, bound = reference(cid)
    assert left_out.sum() <= int(c["cap"] * left_out.size)
    rays, rates = launch(riab, r, default_cells(c["n"], False, angles, dirs, r["walls"]), c["pos"], c["pos_ld"])
    got = rays.transpose(0, 2, 1).reshape(T * B, K).astype(np.float64)          # ray_out is indexed (t K + k) B + b
    ref32 = ref.astype(np.float32).astype(np.float64)
    keep = ~left_out
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref32)                                                # (+0 and -0 compare equal)
        ulps = np.where(keep, err / bc.ulp32(np.where(np.isfinite(ref), ref, 0.0)), 0.0)
        ratio = np.where(keep, err / bound, 0.0)
        bad = keep & ~(err <= bound)
    print(f"bvc-rays {cid}: {int(left_out.sum())} of {left_out.size} left out, worst {np.nanmax(ulps):.2f} ulp, "
          f"worst err / bound {np.nanmax(ratio):.3f}, {int(bad.sum())} outside")
    assert not bad.any(), (f"{cid}: {int(bad.sum())} of {int(keep.sum())} rays outside the bound; first at (position, ray) "
                           f"{tuple(np.argwhere(bad)[0])}: got {got[bad][0]!r}, reference {ref32[bad][0]!r}")
    if "edge_tile" in c or "edge_lane" in c:
        lanes = list(range(c["edge_tile"], T * B)) if "edge_tile" in c else [c["edge_lane"]]
        zeros = (ref[lanes] == 0) & keep[lanes]
        assert zeros.sum() >= len(lanes) * (K // 2 - 4) and (got[lanes][zeros] == 0).all()
    assert np.isfinite(rates[:, :, :]).all() or not c["inside"]


# ----------------------------------------------------------------------------- 2. stage B from the kernel's own rays
def _class_tables(riab, n, mu):
    """The device tables of a BoundaryVectorCells population of the maze with direction windows: the class's own."""
    env = riab.Environment({"walls": bc.MAZE})
    BVs = riab.BoundaryVectorCells(riab.Agent(env), {"n": n})
    bc.tune(BVs, mu)
    BVs._call(None, None)
    dirs_t, rden_t, cells_t, vm_t, inv_t, rows_t, win_t = BVs._table_cache["t"][1]
    return dict(test_dirs=dirs_t, ray_rden=rden_t, cells=cells_t, vm=vm_t, inv_norm=inv_t, K=180), rows_t, win_t


_stage_b_rays = {}


@pytest.mark.parametrize("n", bc.STAGE_B_COUNTS)
@pytest.mark.parametrize("mode", ["allo", "ego", "windows"])
def test_stage_b_from_the_kernels_own_rays(riab, mode, n, monkeypatch):
    monkeypatch.delenv("RIAB_NO_BVC_WINDOWS", raising=False)
    r, (angles, dirs) = bc.room("maze"), bc.table("K180")
    T, B, ld = bc.ROWS["T"], bc.ROWS["B"], bc.ROWS["pos_ld"]
    rs = np.random.RandomState(107)
    pos = r["inside"](rs, T * B).reshape(T, B, 2)
    hd = None
    if mode == "ego":
        a = rs.uniform(0, 2 * np.pi, (T, B))
        hd = bc.f32(np.stack((np.cos(a), np.sin(a)), axis=-1))
    mu = bc.stage_b_cells(n)
    tabs = bc.bvc_tables(r["walls"], angles, dirs, *mu, mode == "ego")
    rows = win = None
    extra = 0.0
    if mode == "windows":
        ctabs, rows, win = _class_tables(riab, n, mu)
        if rows is None:
            assert n < 8            # (a handful of cells can need every direction: then there is nothing to skip)
        else:
            tabs, extra = ctabs, bc.BVC_WINDOW_SHARE
            w = win.cpu().numpy()
            print(f"bvc-stage-b windows n={n}: {int((w.sum(axis=1) > 180).sum())} of {len(w)} windows wrap past K, "
                  f"{w[:, 1].sum() / (180.0 * len(w)):.3f} of the terms issued")
    rays, rates = launch(riab, r, tabs, pos, ld, hd=hd, rows=rows, win=win)
    # the rays do not depend on the cells, the frame or the windows
    key = rays.tobytes()
    assert _stage_b_rays.setdefault("rays", key) == key
    d = rays.transpose(0, 2, 1).reshape(T * B, 180).astype(np.float64)
    flat_hd = None if hd is None else hd.reshape(-1, 2)
    want = bc.stage_b_reference(d, angles, *(mu[i] for i in (0, 1, 2, 3)), hd=flat_hd)                   # (n, P) float64
    host = bc.stage_b_float32(d, bc.bvc_tables(r["walls"], angles, dirs, *mu, mode == "ego"), hd=flat_hd)
    tol = 4 * float(np.abs(host.astype(np.float64) - want).max()) + extra
    got = rates.transpose(1, 0, 2).reshape(n, T * B).astype(np.float64)
    worst = float(np.abs(got - want).max())
    print(f"bvc-stage-b {mode} n={n} (split {bc.kernel_split(n, T * B)}): worst |got - ref| {worst:.3e}, bound {tol:.3e}, "
          f"ratio {worst / tol:.3f}")
    assert np.isfinite(got).all() and worst <= tol


def test_a_window_wraps_past_k(riab):
    """Among the windowed cases above there is a window that wraps past K (the kernel's `k + 4 - Kw` step)."""
    wraps = 0
    for n in bc.STAGE_B_COUNTS:
        _tabs, rows, win = _class_tables(riab, n, bc.stage_b_cells(n))
        if win is not None:
            w = win.cpu().numpy()
            wraps += int((w.sum(axis=1) > 180).sum())
    assert wraps >= 1


# ----------------------------------------------------------------------------- 3. through the classes
def assert_rates(got, ref, scale=1.0, floor=0.0):
    """The project's check (tests/test_gpu_parity.py): |got - ref| <= RTOL |ref| + floor RTOL scale."""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert got.shape == ref.shape
    tol = RTOL * np.abs(ref) + floor * RTOL * scale + 1e-37
    bad = ~(np.abs(got - ref) <= tol)
    print(f"bvc-classes: worst err / tol {np.nanmax(np.abs(got - ref) / tol):.3f}")
    assert not bad.any(), (f"{bad.sum()} / {bad.size} outside tolerance at (cell, position) {np.argwhere(bad)[:6].tolist()}; "
                           f"worst abs err {np.nanmax(np.abs(got - ref)):.3e}")


@pytest.mark.parametrize("frame", ["allocentric", "egocentric"])
def test_boundary_vector_cells_on_the_edges(riab, frame):
    pos, hd = bc.class_positions()
    np.random.seed(13)
    for walls in bc.CLASS_WALLS:        # (why not the maze: see there)
        env = riab.Environment({"walls": [np.asarray(w).tolist() for w in walls]})
        BVs = riab.BoundaryVectorCells(riab.Agent(env), {"n": 40, "reference_frame": frame})
        ego = frame == "egocentric"
        got = BVs.get_state(evaluate_at=None, pos=pos, **(dict(head_direction=hd) if ego else {}))
        ref = orc.bvc(pos, env.walls, BVs.tuning_distances, BVs.tuning_angles, BVs.sigma_distances, BVs.sigma_angles,
                      head_direction=hd if ego else None)
        assert np.isfinite(ref).all() and (ref[:, :4] > 0.01).any()
        assert_rates(got, ref, floor=1.0)


def test_field_of_view_bvcs_on_the_edges(riab):
    pos, hd = bc.class_positions()
    env = riab.Environment()
    F = riab.FieldOfViewBVCs(riab.Agent(env))
    got = F.get_state(evaluate_at=None, pos=pos, head_direction=hd)
    ref = orc.bvc(pos, env.walls, F.tuning_distances, F.tuning_angles, F.sigma_distances, F.sigma_angles, head_direction=hd)
    assert np.isfinite(ref).all() and (ref[:, :4] > 0.01).any()
    assert_rates(got, ref, floor=1.0)
