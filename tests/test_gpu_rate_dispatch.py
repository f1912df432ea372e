"""Every slot of the rate kernels' dispatch tables (riab_rates.hip: launch_rate, launch_stream_cell) on the GPU.

The host picks a kernel from a table by (spike mode, streamed stores) for the wide kernel, by spike mode for the generic
one and by (reserving shape, spikes, LONG) for the row-following one, for every functor the visitors of description,
geometry and population kind produce.  The other GPU tests reach the functors' values; these reach every SLOT with the
smallest shapes that are ragged against the cell group: a slot that held another variant's kernel (explicit uniforms
served by the Philox kernel, the spike and no-spike entries swapped, ...) fails here."""
import os

import numpy as np
import pytest
import torch

from oracle import riab_oracle as orc
from tests.test_gpu_fused import MAZE, _gc, _hdc, _pc, _run

pytestmark = pytest.mark.gpu

N = 5            # cells: ragged against the wide kernel's 4 (PlaceCells, GridCells) and 16 (HeadDirectionCells) per group
SEED, STEP0, POP_ID, ID0, DT = 0x1234567800000321, 5, 3, 4096, 0.05
WALLS = [[0, 0, 1, 0], [1, 0, 1, 1], [1, 1, 0, 1], [0, 1, 0, 0], [0.5, 0.1, 0.5, 0.6]]   # the box and one internal wall


@pytest.fixture(scope="module")
def riab():
    assert torch.cuda.is_available(), "these tests need the GPU"
    import ratinabox_amd
    return ratinabox_amd


@pytest.fixture(scope="module")
def rows():
    """positions and head directions of 1024 agents over two time rows, (2, 2, 1024) each; the uniforms of (2, N, 1024)"""
    rs = np.random.RandomState(11)
    pos = rs.uniform(0.02, 0.98, (2, 2, 1024)).astype(np.float32)
    ang = rs.uniform(0, 2 * np.pi, (2, 1024))
    hd = np.stack((np.cos(ang), np.sin(ang)), 1).astype(np.float32)
    u = rs.uniform(0, 1, (2, N, 1024)).astype(np.float32)
    return pos, hd, u


def _tables():
    rs = np.random.RandomState(3)
    c = rs.uniform(0.1, 0.9, (N, 2))
    pc = np.concatenate((c, np.full((N, 1), -np.log2(np.e) / (2 * 0.2 ** 2))), 1).astype(np.float32)
    gc = rs.uniform(-3, 3, (N, 9)).astype(np.float32)
    a = rs.uniform(0, 2 * np.pi, N)
    hdc = np.stack((np.cos(a), np.sin(a), np.full(N, np.log2(np.e) / 0.5 ** 2)), 1).astype(np.float32)
    return pc, gc, hdc


# functor families: (kind, description, geometry, periodic) — every description, every GX
FAMILIES = [("place", d, g, p) for d in ("gaussian", "gaussian_threshold", "diff_of_gaussians", "top_hat")
            for g, p in (("euclidean", False), ("line_of_sight", False), ("geodesic", False), ("euclidean", True))]
FAMILIES += [("grid", "rectified_cosines", None, False), ("grid", "shifted_cosines", None, False), ("hdc", None, None, False)]
# kernel forms: (B, T): the wide kernel with ordinary stores, with streamed ones (a one-row launch), the generic kernel
FORMS = {"wide": (1024, 2), "wide_one_row": (1024, 1), "generic": (8, 2)}


def _call(riab, fam, form, spk, rows):
    """-> (rates (T, N, B), spike bytes (T, N, B) pre-filled with 0xEE, the uniforms the call was given or None)"""
    from ratinabox_amd import ops
    L = riab._lib
    kind, desc, geom, periodic = fam
    B, T = FORMS[form]
    pos, hd, u = rows
    dev = "cuda"
    # (the B agents are the first B of the 1024: the forms see the same positions; row pitch = B)
    p = torch.tensor(np.ascontiguousarray(pos[:T, :, :B]), device=dev)     # (T, 2, B)
    h = torch.tensor(np.ascontiguousarray(hd[:T, :, :B]), device=dev)
    px, py = p[:, 0].contiguous(), p[:, 1].contiguous()
    hx, hy = h[:, 0].contiguous(), h[:, 1].contiguous()
    rates = torch.full((T, N, B), -7.0, dtype=torch.float32, device=dev)
    spikes = torch.full((T, N, B), 0xEE, dtype=torch.uint8, device=dev)
    uin = torch.tensor(np.ascontiguousarray(u[:T, :, :B]), device=dev)
    io = L.RiabRateIO()
    io.pos_x, io.pos_y, io.hd_x, io.hd_y = px.data_ptr(), py.data_ptr(), hx.data_ptr(), hy.data_ptr()
    io.pos_ld, io.T, io.B = B, T, B
    io.rates = rates.data_ptr()
    io.spikes = spikes.data_ptr() if spk != "none" else None
    io.u_in = uin.data_ptr() if spk == "explicit" else None
    io.dt, io.min_fr, io.max_fr = DT, 2.0, 12.0
    io.seed, io.step0, io.agent_id0, io.pop_id = SEED, STEP0, ID0, POP_ID
    pc, gc, hdc = _tables()
    s = L.current_stream()
    if kind == "place":
        tab = torch.tensor(pc, device=dev)
        walls = torch.tensor(WALLS, dtype=torch.float64, device=dev)
        env = ops._env_struct(walls, [0.0, 1.0, 0.0, 1.0, 1.0], periodic)
        rc = L.lib.riab_place_cells(env, io, L.ptr(tab), N, L.PC_DESCRIPTIONS[desc], L.GEOMETRIES[geom], 0.3, s)
    elif kind == "grid":
        tab = torch.tensor(gc, device=dev)
        rc = L.lib.riab_grid_cells(io, L.ptr(tab), N, L.GC_DESCRIPTIONS[desc], 0.2, s)
    else:
        tab = torch.tensor(hdc, device=dev)
        rc = L.lib.riab_head_direction_cells(io, L.ptr(tab), N, s)
    assert rc == 0, (fam, form, spk, rc)
    torch.cuda.synchronize()
    return rates.cpu().numpy(), spikes.cpu().numpy(), (u[:T, :, :B] if spk == "explicit" else None)


@pytest.mark.parametrize("fam", FAMILIES, ids=["-".join(str(x) for x in f if x not in (None, False)) + ("-periodic" if f[3] else "")
                                               for f in FAMILIES])
def test_every_wide_and_generic_table_slot(riab, rows, fam):
    """(spike mode) x (kernel form) for one functor: the rates are the same bits in all nine calls (the forms share the
    agents' positions), no call without spikes touches the spike rows, and the spike bytes are the exactly-specified rule
    on the call's own rates with the host-regenerated Philox uniforms, or with the explicit ones it was handed."""
    ref = None
    for form, (B, T) in FORMS.items():
        for spk in ("none", "philox", "explicit"):
            fr, sp, u = _call(riab, fam, form, spk, rows)
            assert np.isfinite(fr).all() and (fr != -7.0).all(), (form, spk)   # (every element written; a difference of
            # gaussians and shifted cosines leave [min_fr, max_fr] by their definitions)
            if ref is None:
                ref = fr                                     # wide, two rows, no spikes
                assert np.ptp(ref) > 0
            np.testing.assert_array_equal(fr, ref[:T, :, :B], err_msg=f"{form} {spk}")
            if spk == "none":
                assert (sp == 0xEE).all(), (form, spk)
                continue
            for t in range(T):
                uu = u[t] if spk == "explicit" else orc.spike_uniforms(SEED, STEP0 + t, POP_ID, N, B, agent_id0=ID0)
                want = orc.spikes_f32(fr[t], uu, DT)
                assert np.array_equal(sp[t].astype(bool), want), (form, spk, t)
                assert (sp[t] <= 1).all()
            assert sp.sum() > 0


def test_wide_gaussian_rates_match_the_oracle(riab, rows):
    """... and the bits all those calls agree on are the oracle's values (1e-5 relative, as tests/test_gpu_parity.py)"""
    fr, _sp, _u = _call(riab, ("place", "gaussian", "euclidean", False), "wide", "none", rows)
    pc, _gc_, _hd = _tables()
    pos = rows[0]
    for t in range(2):
        want = orc.place_cells(orc.EnvSpec(walls=np.zeros((0, 2, 2))), np.stack((pos[t, 0], pos[t, 1]), -1).astype(np.float64),
                               pc[:, :2].astype(np.float64), np.full(N, 0.2))
        np.testing.assert_allclose(fr[t], 2.0 + 10.0 * want, rtol=1e-5, atol=1e-6)


# ---- the row-following kernel: [reserving shape][spikes][LONG] --------------------------------------------------------
GATED_POPS = {"place": lambda spk: _pc(9, save_spikes=spk), "place_los": lambda spk: _pc(9, wall_geometry="line_of_sight", save_spikes=spk),
              "grid": lambda spk: _gc(9, save_spikes=spk), "hdc": lambda spk: _hdc(9, save_spikes=spk)}
_chunked = {}


def _reference(riab, kind, spk, T):
    """the Python-driven chunked pipeline, once per (population, spikes, rows)"""
    key = (kind, spk, T)
    if key not in _chunked:
        env = {"walls": MAZE} if kind == "place_los" else None
        _chunked[key] = _run(riab, False, 256, GATED_POPS[kind](spk), [("sim", T)], env)[:3]
    return _chunked[key]


@pytest.mark.parametrize("gate", ["reserved", "always"])
@pytest.mark.parametrize("spk", [False, True], ids=["nospikes", "spikes"])
@pytest.mark.parametrize("T", [3, 257])
@pytest.mark.parametrize("kind", sorted(GATED_POPS))
def test_every_gated_table_slot(riab, kind, T, spk, gate):
    """256 agents, 9 cells (ragged against the gated kernel's 8 / 4 / 16 per group), 3 rows and 257 (the LONG name), in the
    reserving shape and behind the started gate, with and without spikes: trajectory, rates and spikes bit for bit those
    of the chunked pipeline.  (Line-of-sight place cells are refused the reserving shape: they take the gate in both.)"""
    os.environ["RIAB_GATE"] = gate
    try:
        env = {"walls": MAZE} if kind == "place_los" else None
        t_a, fr_a, sp_a, ag = _run(riab, True, 256, GATED_POPS[kind](spk), [("sim", T)], env)
        assert ag._streamer is not None and ag.diagnostics["pipeline_timeouts"] == 0
    finally:
        os.environ.pop("RIAB_GATE", None)
    t_b, fr_b, sp_b = _reference(riab, kind, spk, T)
    np.testing.assert_array_equal(t_a, t_b)
    np.testing.assert_array_equal(fr_a, fr_b)
    np.testing.assert_array_equal(sp_a, sp_b)
    if spk:
        assert sp_a.sum() > 0
