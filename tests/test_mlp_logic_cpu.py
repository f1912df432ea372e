"""No-GPU checks of what a riab_mlp_forward call decides before it launches: csrc/riab_mlp_logic.h — the text the library
compiles — built for the host with g++ behind tests/native/mlp_logic_host.cpp, a stand-alone program that reads facts and
prints decisions.  The table restates the rules of the header comments of csrc/riab_mlp.hip; the coverage test proves that
the case list of tests/mlp_path_cases.py (what tests/test_gpu_mlp_paths.py runs) reaches every form, by name."""
import os
import subprocess

import pytest

from tests import mlp_path_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, ETOOBIG = -1, -2, -3
CUS = 256
LISTS = ("vec", "koff", "vec0", "passes", "mti", "tiles")


@pytest.fixture(scope="module")
def decide(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mlp_logic") / "mlp_logic_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "ratinabox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "mlp_logic_host.cpp"), "-o", exe], check=True)

    def run(*rows):
        """one dict per row of facts (values: int, or a list of int for the per-layer / per-input / per-pass fields)"""
        out = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(rows)
        res = []
        for line in out:
            d = {}
            for w in line.split():
                k, v = w.split("=")
                d[k] = ([] if v == "-" else [int(x) for x in v.split(",")]) if k in LISTS else int(v)
            res.append(d)
        return res if len(res) > 1 else res[0]
    return run


def _has(d, **kw):
    assert {k: d.get(k) for k in kw} == kw, d


# ------------------------------------------------------------------------------------------------------------ the table
def test_kernel_and_pass_thresholds(decide):
    """mlp_kernel<MAXT>: the tiles of the widest activation carried (thresholds 32 and 64; one layer: its rows of one
    128-row pass); mlp_first_layer<MT> per pass from the rows left (32, 64); passes of 128 rows only for a single layer"""
    for n_out, maxt, passes in ((1, 1, [1]), (32, 1, [1]), (33, 2, [2]), (64, 2, [2]), (65, 4, [4]), (128, 4, [4]),
                                (129, 4, [4, 1]), (160, 4, [4, 1]), (161, 4, [4, 2]), (192, 4, [4, 2]), (193, 4, [4, 4]),
                                (256, 4, [4, 4]), (257, 4, [4, 4, 1]), (300, 4, [4, 4, 2]), (228, 4, [4, 4])):
        _has(decide(f"in=20 layer=20:{n_out}"), rc=0, maxt=maxt, passes=passes, mti=[], tiles=[])
    # several layers: the widest HIDDEN width decides, the last layer's rows do not; layer 0 is one pass of its own rows
    for hidden, maxt, mt0 in (([20], 1, 1), ([32, 32], 1, 1), ([20, 33], 2, 1), ([33, 20], 2, 2), ([64], 2, 2), ([20, 65], 4, 1),
                              ([33, 128], 4, 2), ([64, 96], 4, 2), ([65], 4, 4), ([128, 20], 4, 4)):
        ws = [20] + hidden + [300]
        d = decide("in=20 " + " ".join(f"layer={a}:{b}" for a, b in zip(ws, ws[1:])))
        _has(d, rc=0, maxt=maxt, passes=[mt0], mti=[(w + 31) // 32 for w in hidden], tiles=[(w + 31) // 32 for w in ws[2:]])


def test_block_grid_and_lds(decide):
    """nw = 4 iff ceil(B / 128) * T >= the compute units; blocks of 32 nw positions; LDS: the 16 KB W slabs + 2 x 16 x 32 nw floats"""
    for T, B, cus, nw in ((1, 4096, 256, 1), (8, 4096, 256, 4), (255, 128, 256, 1), (256, 128, 256, 4), (128, 132, 256, 4),
                          (127, 132, 256, 1), (128, 128, 256, 1), (2, 132, 256, 1), (2, 132, 4, 4), (1, 4, 1, 4), (65535, 4, 65536, 1),
                          (3, 388, 12, 4), (3, 388, 13, 1)):
        assert mc.expected_nw(T, B, cus) == nw
        _has(decide(f"in=20 layer=20:7 T={T} B={B} cus={cus}"), rc=0, nw=nw, grid_x=-(-B // (32 * nw)), grid_z=T,
             lds=16384 + 2 * 16 * 32 * nw * 4)


def test_read_widths(decide):
    """vec iff the base is 16-byte aligned and n_in % 4 == 0; vec0 iff vec and koff % 4 == 0; koff: the running sum"""
    _has(decide("in=3 in=17 layer=20:7"), vec=[1], koff=[0, 3], vec0=[1, 0])
    _has(decide("in=16 in=4 layer=20:7"), vec=[1], koff=[0, 16], vec0=[1, 1])
    _has(decide("in=5 in=19 in=108 layer=132:7"), vec=[1], koff=[0, 5, 24], vec0=[1, 0, 1])
    _has(decide("in=16 in=3 layer=19:7"), vec=[0], vec0=[0, 0])
    for mod in (4, 8, 12):
        _has(decide(f"in=16 in=4 layer=20:7:1:0:{mod}"), vec=[0], vec0=[0, 0])
    _has(decide("in=20 layer=20:33 layer=33:64:1:0:0 layer=64:64:1:0:4 layer=64:5"), vec=[1, 0, 0, 1], mti=[2, 2, 2], tiles=[2, 2, 1])


def test_errors_in_the_order_of_the_checks(decide):
    ok = "in=10 layer=10:20:1:2 layer=20:4"
    _has(decide(ok), rc=0)
    for facts, rc in (
            # null pointers and non-positive sizes
            (ok + " out_null=1", EINVAL), (ok + " T=0", EINVAL), (ok + " B=0", EINVAL), (ok + " B=-4", EINVAL),
            (ok + " n_inputs=0", EINVAL), (ok + " n_layers=0", EINVAL), ("in=10:0:1 layer=10:4", EINVAL),
            ("in=4 in=0 in=6 layer=10:4", EINVAL), ("in=10 layer=10:0", EINVAL), ("in=10 layer=10:4:1:0:0:1", EINVAL),
            # a broken width chain, inputs that do not add up to layer 0's n_in, an unknown activation
            ("in=10 layer=10:20 layer=21:4", EINVAL), ("in=4 in=5 layer=10:4", EINVAL), ("in=11 layer=10:4", EINVAL),
            ("in=10 layer=10:20:1:6", EINVAL), ("in=10 layer=10:20:1:-1", EINVAL),
            # alignment
            (ok + " B=6", EALIGN), (ok + " out_mod16=8", EALIGN), ("in=10:4 layer=10:4", EALIGN),
            # limits
            (" ".join(["in=1"] * 9) + " layer=9:4", ETOOBIG), ("in=10 layer=10:8 " + " ".join(["layer=8:8"] * 8), ETOOBIG),
            ("in=10 layer=10:129 layer=129:4", ETOOBIG), (ok + " T=65536", ETOOBIG), (ok + " T=65535", 0),
            ("in=10 layer=10:128 layer=128:129", 0),
            # the order: counts before entries; sizes, then the chain, then the hidden limit, then alignment
            (ok + " T=65536 out_null=1", EINVAL), (" ".join(["in=1:0:1"] * 9) + " layer=9:4", ETOOBIG),
            ("in=10:4 layer=10:129 layer=129:4", ETOOBIG), ("in=10 layer=10:129 layer=128:4", EINVAL),
            ("in=11 layer=10:129 layer=129:4", EINVAL), (ok + " B=6 T=65536", ETOOBIG), ("in=10:4 layer=10:20:1:7", EINVAL)):
        assert decide(facts)["rc"] == rc, facts


# ------------------------------------------------------------------------------------------------------------ coverage
def _k_class(K):
    return "K<4" if K < 4 else "4<=K<16" if K < 16 else "K=16" if K == 16 else "K>16 ragged" if K % 16 else "K>16 whole"


PAIRS = [(1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 4)]
REQUIRED = (
    [f"nw={nw}: mlp_first_layer<{mt}> in mlp_kernel<{maxt}>" for nw in (1, 4) for maxt, mt in PAIRS]
    + [f"several passes, the last with {mt} tile(s)" for mt in (1, 2, 4)]
    + [f"vec0={v} at {k}" for v in (0, 1) for k in ("K<4", "4<=K<16", "K=16", "K>16 ragged")]
    + [f"mlp_reg_tile<{mti}, vec={v}>" for v in (0, 1) for mti in (1, 2, 3, 4)]
    + [f"register layer with n_in % 32 != 0, vec={v}" for v in (0, 1)]
    + ["last layer with more tiles than maxt"]
    + [f"bias {s} on the {w} layer" for s in ("present", "absent") for w in ("first", "middle", "last")]
    + ["vec=0 by the base address alone"]
    + [f"activation {a}" for a in range(6)])


def _reached(decide, cases):
    """the names of REQUIRED's kind that the cases reach at 256 compute units, over every launch shape"""
    runs = [(c, nw, T, B) for c in cases for nw, T, B in mc.launch_shapes(CUS)]
    if not runs:
        return set()
    res = decide(*(mc.facts_line(c, T, B, CUS) for c, _nw, T, B in runs))
    got = set()
    for (c, nw, T, B), d in zip(runs, res if isinstance(res, list) else [res]):
        assert d["rc"] == 0 and d["nw"] == nw == mc.expected_nw(T, B, CUS), (c.name, T, B, d)
        n_l = len(c.layers)
        for mt in d["passes"]:
            got.add(f"nw={nw}: mlp_first_layer<{mt}> in mlp_kernel<{d['maxt']}>")
        if len(d["passes"]) > 1:
            got.add(f"several passes, the last with {d['passes'][-1]} tile(s)")
        for K, v in zip(c.inputs, d["vec0"]):
            got.add(f"vec0={v} at {_k_class(K)}")
        for i, (k, _m) in enumerate(mc.widths(c)):
            L = c.layers[i]
            where = ["first"] * (i == 0) + ["last"] * (i == n_l - 1) + ["middle"] * (0 < i < n_l - 1)
            got.update(f"bias {'present' if L.bias else 'absent'} on the {w} layer" for w in where)
            got.add(f"activation {L.act}")
            if L.w_off and k % 4 == 0 and d["vec"][i] == 0:
                got.add("vec=0 by the base address alone")
            if i >= 1:
                got.add(f"mlp_reg_tile<{d['mti'][i - 1]}, vec={d['vec'][i]}>")
                if k % 32:
                    got.add(f"register layer with n_in % 32 != 0, vec={d['vec'][i]}")
        if n_l > 1 and d["tiles"][-1] > d["maxt"]:
            got.add("last layer with more tiles than maxt")
    return got


def test_the_cases_reach_every_path(decide):
    missing = [name for name in REQUIRED if name not in _reached(decide, mc.CASES)]
    assert not missing, "no case of tests/mlp_path_cases.py reaches: " + "; ".join(missing)


def test_every_case_is_the_only_one_that_reaches_something(decide):
    """deleting any one case makes the coverage test fail (so none is there by habit)"""
    for i, c in enumerate(mc.CASES):
        got = _reached(decide, mc.CASES[:i] + mc.CASES[i + 1:])
        assert [name for name in REQUIRED if name not in got], f"{c.name} could be deleted without losing a path"


def test_flat_weights_force_four_byte_reads(decide):
    """the all-flat rerun of test_gpu_mlp_paths.py (every base 4 mod 16): no layer and no input keeps 16-byte reads"""
    for c in mc.CASES:
        d = decide(mc.facts_line(c, 2, 132, CUS, flat=True))
        assert not any(d["vec"]) and not any(d["vec0"]), (c.name, d)
