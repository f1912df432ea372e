"""No-GPU checks of the rate-map feature: the host definition (utils.bin_data_for_histogramming) against the
reference's own results, the edge builder, the chunk-segment helper, the ABI of the riab_history_* entry points and
the class-level errors."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from tests import ratemap_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "riab_hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ratemap_reference.npz")
NEW_SYMBOLS = {"riab_history_bin_index": 12, "riab_history_rate_map_workspace": 4, "riab_history_rate_map": 11,
               "riab_history_rate_map_finish": 8}


@pytest.fixture(scope="module")
def G():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def L():
    from ratinabox_amd import _lib
    return _lib


def test_host_binning_equals_the_reference_bit_for_bit(G):
    from ratinabox_amd import utils
    pos = G["pos"].astype(np.float64)
    for tag, dx in (("05", 0.05), ("10", 0.1)):
        for name, w in (("rate", G["fr"]), ("spike", G["spikes"])):
            w = w.astype(np.float64)
            for c in range(w.shape[1]):
                m, zero = utils.bin_data_for_histogramming(pos, G["extent"], dx, weights=w[:, c], norm_by_bincount=True,
                                                           return_zero_bins=True)
                assert np.array_equal(m, G[f"{name}_norm_{tag}"][c]) and np.array_equal(zero, G[f"zero_bins_{tag}"])
                s = utils.bin_data_for_histogramming(pos, G["extent"], dx, weights=w[:, c])
                assert np.array_equal(s, G[f"{name}_sum_{tag}"][c])
        assert np.array_equal(utils.bin_data_for_histogramming(pos, G["extent"], dx), G[f"heatmap_{tag}"])
        # the unnormalised call can report its empty bins too
        h, zero = utils.bin_data_for_histogramming(pos, G["extent"], dx, return_zero_bins=True)
        assert np.array_equal(h, G[f"heatmap_{tag}"]) and np.array_equal(zero, G[f"zero_bins_{tag}"])
    with pytest.raises(NotImplementedError):
        utils.bin_data_for_histogramming(pos[:, 0], (0.0, 1.0), 0.05)


def test_oracle_equals_the_reference(G):
    """The tests' float64 restatement, on the fixture laid out as history rows, is the reference's result."""
    T = len(G["pos"])
    traj = np.zeros((T, 8, 4), dtype=np.float32)
    traj[:, 0, 0], traj[:, 1, 0] = G["pos"][:, 0], G["pos"][:, 1]
    rows = np.zeros((T, 10, 4), dtype=np.float32)
    rows[:, :, 0] = G["fr"]
    ex, ey = orc.edges(G["extent"], 0.05)
    maps, zero, cnt = orc.rate_maps(traj, rows, 1, ex, ey, True)
    assert np.array_equal(maps, G["rate_norm_05"]) and np.array_equal(zero, G["zero_bins_05"])
    assert np.array_equal(cnt, G["heatmap_05"])


@pytest.mark.parametrize("extent, dx, nx, ny", [((0, 1, 0, 1), 0.05, 20, 20), ((0, 1, 0, 1), 0.04, 25, 25),
                                                 ((0, 2, 0, 1), 0.05, 40, 20), ((0, 0.3, 0, 0.2), 0.1, 3, 3),
                                                 ((-0.5, 0.5, -0.25, 0.25), 0.05, 20, 10)])
def test_edge_builder(extent, dx, nx, ny):
    from ratinabox_amd import utils
    ex, ey = utils.histogram_bin_edges(extent, dx)
    assert ex.dtype == np.float64 and (len(ex) - 1, len(ey) - 1) == (nx, ny)
    assert np.array_equal(ex, np.arange(extent[0], extent[1] + dx, dx))
    assert np.array_equal(ey, np.arange(extent[2], extent[3] + dx, dx))
    if extent == (0, 0.3, 0, 0.2):
        assert ex[-1] == 0.30000000000000004
    if extent[0] == -0.5:   # the last edges lie below the extent: a position on the far wall is outside the map
        assert ex[-1] == 0.4999999999999998 and ey[-1] == 0.2499999999999999
        assert orc.searchsorted_bins([0.5], ex)[0] == -1


def test_histogram2d_is_the_searchsorted_rule():
    """The statement the kernel implements: np.histogram2d with explicit edges == searchsorted(side='right') - 1 with a
    closed last bin, points on edges included."""
    rng = np.random.RandomState(0)
    ex, ey = orc.edges((0, 0.3, 0, 0.2), 0.1)
    x = np.concatenate((rng.uniform(-0.05, 0.35, 980), ex, [np.nan, -0.0, np.nextafter(ex[-1], 1.0)] * 5, [0.1]))[:1000]
    y = rng.uniform(-0.05, 0.25, len(x))
    y[:len(ey)] = ey
    h = np.histogram2d(x, y, bins=[ex, ey])[0]
    kx, ky = orc.searchsorted_bins(x, ex), orc.searchsorted_bins(y, ey)
    ref = np.zeros_like(h)
    for a, b in zip(kx, ky):
        if a >= 0 and b >= 0:
            ref[a, b] += 1
    assert np.array_equal(h, ref)


def _covered(segs, fa, fp):
    rows = []
    for ca, ra, cp, rp, n in segs:
        assert n > 0 and 0 <= ra and ra + n <= fa[ca] and 0 <= rp and rp + n <= fp[cp]
        ga, gp = sum(fa[:ca]) + ra, sum(fp[:cp]) + rp
        assert ga == gp
        rows.extend(range(ga, ga + n))
    return rows


@pytest.mark.parametrize("fa, fp", [([37, 50], [4096]), ([1, 1, 85], [87]), ([87], [87]), ([37, 50, 5], [37, 50, 5]),
                                     ([3, 0, 4], [2, 5]), ([5, 2], [1, 1, 1, 1, 1, 1, 1])])
def test_history_segments_exhaustive(fa, fp):
    from ratinabox_amd._ratemap import history_segments
    total = min(sum(fa), sum(fp))
    for start, stop in itertools.combinations_with_replacement(range(total + 1), 2):
        segs = history_segments(fa, fp, start, stop)
        assert _covered(segs, fa, fp) == list(range(start, stop))
        # as few pieces as the chunk boundaries allow: a new piece starts only where one of the histories changes chunk
        for (ca, ra, cp, rp, n), nxt in zip(segs, segs[1:]):
            assert ra + n == fa[ca] or rp + n == fp[cp]
    assert history_segments(fa, fp, 3, 3) == [] and history_segments(fa, fp, 4, 2) == []
    with pytest.raises(ValueError):
        history_segments(fa, fp, 0, total + 1)
    with pytest.raises(ValueError):
        history_segments(fa, fp, -1, 1)


def test_new_symbols_declared_exported_prototyped(L):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, argc in NEW_SYMBOLS.items():
        m = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in riab_hip.h"
        assert len(m.group(1).split(",")) == argc
        assert hasattr(L.lib, name) and len(L.PROTOTYPES[name][1]) == argc
    raw = open(HEADER).read()
    assert int(re.search(r"#define RIAB_ABI_VERSION (\d+)", raw).group(1)) == 11 == L.ABI_VERSION == L.lib.riab_abi_version()
    for name, val in (("RIAB_RATEMAP_MAX_BINS", L.RATEMAP_MAX_BINS), ("RIAB_RATEMAP_FP32_RUN", L.RATEMAP_FP32_RUN)):
        assert int(re.search(rf"#define {name} (\d+)", raw).group(1)) == val
    assert int(re.search(r"#define RIAB_RATEMAP_DROPPED (0x[0-9A-Fa-f]+)", raw).group(1), 16) == L.RATEMAP_DROPPED
    assert L.RATEMAP_MAX_BINS >= 4096


def test_argument_errors_before_launch(L):
    """Every refusal of the riab_history_* entry points is produced by validation alone: no device needed."""
    p, q = C.c_void_p(4096), C.c_void_p(4096 + 4)
    ex = np.arange(0, 1.05, 0.05)
    ey = np.arange(0, 1.05, 0.05)
    X, Y = ex.ctypes.data, ey.ctypes.data

    def bin_index(hist=p, T=1, B=8, n_real=8, ex_=X, nx=20, ey_=Y, ny=20, dev=p, ids=p, counts=p):
        return L.lib.riab_history_bin_index(hist, T, B, n_real, ex_, nx, ey_, ny, dev, ids, counts, None)
    for null in ("hist", "ex_", "ey_", "dev", "ids", "counts"):
        assert bin_index(**{null: None}) == L.EINVAL
    assert bin_index(n_real=9) == L.EINVAL and bin_index(T=-1) == L.EINVAL
    assert bin_index(B=6, n_real=6) == L.EALIGN and bin_index(hist=q) == L.EALIGN and bin_index(ids=q) == L.EALIGN
    assert bin_index(nx=0) == L.EINVAL and bin_index(ny=0) == L.EINVAL          # fewer than two edges
    flat = ex.copy()
    flat[7] = flat[6]
    assert bin_index(ex_=flat.ctypes.data) == L.EINVAL                            # not strictly increasing
    down = ey[::-1].copy()
    assert bin_index(ey_=down.ctypes.data) == L.EINVAL
    nan = ex.copy()
    nan[3] = np.nan
    assert bin_index(ex_=nan.ctypes.data) == L.EINVAL
    big = np.arange(0, 66.0)                                                      # 65 x 65 bins
    assert bin_index(ex_=big.ctypes.data, nx=65, ey_=big.ctypes.data, ny=65) == L.EUNSUPPORTED
    assert bin_index(T=1 << 40) == L.ETOOBIG
    assert bin_index(T=0) == 0                                                    # nothing to do, nothing launched

    def rate_map(rows=p, spikes=0, T=1, n=3, B=8, ids=p, nb=400, sums=p, ws=p, wsn=1 << 20):
        return L.lib.riab_history_rate_map(rows, spikes, T, n, B, ids, nb, sums, ws, wsn, None)
    for null in ("rows", "ids", "sums", "ws"):
        assert rate_map(**{null: None}) == L.EINVAL
    assert rate_map(n=0) == L.EINVAL and rate_map(nb=0) == L.EINVAL and rate_map(wsn=5) == L.EINVAL
    assert rate_map(B=6) == L.EALIGN and rate_map(rows=q) == L.EALIGN and rate_map(sums=q) == L.EALIGN
    assert rate_map(rows=q, spikes=1, T=0) == 0                                   # spike rows need 4-byte alignment only
    assert rate_map(nb=L.RATEMAP_MAX_BINS + 1) == L.EUNSUPPORTED and rate_map(T=1 << 40) == L.ETOOBIG
    assert rate_map(T=0) == 0

    ws = L.lib.riab_history_rate_map_workspace
    assert ws(256, 1024, 4096, 400) >= 1024 * 400 and ws(0, 4, 8, 400) == 0
    assert ws(1, 0, 8, 400) == L.EINVAL and ws(1, 4, 6, 400) == L.EALIGN and ws(1, 4, 8, 4097) == L.EUNSUPPORTED
    assert ws(3, 33, 68, 6) % (33 * 6) == 0

    fin = L.lib.riab_history_rate_map_finish
    assert fin(None, p, 2, 400, 1, p, p, None) == L.EINVAL and fin(p, None, 2, 400, 1, p, p, None) == L.EINVAL
    assert fin(p, p, 2, 400, 1, None, p, None) == L.EINVAL and fin(p, p, 2, 0, 1, p, p, None) == L.EINVAL
    assert fin(q, p, 2, 400, 1, p, p, None) == L.EALIGN and fin(p, p, 2, 4097, 1, p, p, None) == L.EUNSUPPORTED


def test_class_level_errors_on_a_cpu_agent():
    import ratinabox_amd as riab
    np.random.seed(0)
    env = riab.Environment({})
    ag = riab.Agent(env, {"n_agents": 8, "device": "cpu"})
    pcs = riab.PlaceCells(ag, {"n": 4})
    with pytest.raises(ValueError, match="no recorded rates"):
        pcs.get_rate_map()
    with pytest.raises(ValueError, match="no recorded spikes"):
        pcs.get_rate_map_tensor(spikes=True)
    with pytest.raises(ValueError, match="method"):
        pcs.get_rate_map(method="neither")
    with pytest.raises(ValueError, match="no history"):
        ag.get_position_heatmap()
    # histories of different lengths, and a position agent of another batch size
    import torch
    pcs._hist_fr.reserve(3)
    with pytest.raises(ValueError, match="one position per recorded row"):
        pcs.get_rate_map()
    other = riab.Agent(env, {"n_agents": 16, "device": "cpu"})
    with pytest.raises(ValueError, match="batch size"):
        pcs.get_rate_map(position_data_agent=other)
    assert torch.is_tensor(pcs._hist_fr.chunks[0])
