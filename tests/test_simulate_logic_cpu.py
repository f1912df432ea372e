"""No-GPU checks of what a riab_simulate call decides before it launches anything: csrc/riab_simulate_logic.h — the text the
library compiles — built for the host with g++ behind tests/native/simulate_logic_host.cpp, a stand-alone program that reads
facts and prints decisions.  The expected values restate the rules of DESIGN.md 3.8; test_gpu_fused.py checks that real
calls report the same forms and launch counts."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, ONE_KERNEL, CHUNKS, SERIAL, POPULATIONS, HEAD_AND_PIECES = range(6)   # RIAB_FORM_*
ALWAYS, WHEN_BUSY, RESERVED = range(3)                                      # RIAB_GATE_*
PLACE, GRID, HDC, BVC, FF = 0, 1, 2, 3, 5                                   # RIAB_POP_*
EUNSUPPORTED = -4


def pop(kind, n, spikes=0, supported=1):
    return f"pop={kind}:{n}:{spikes}:{supported}"


ONE = pop(PLACE, 8)          # one streamable population
TWO = f"{pop(PLACE, 512)} {pop(HDC, 4)} B=2048"   # 512 x 2048 x 4 bytes per row: 645 ns at the built-in 6.5 TB/s
# default mode, a second stream, the earlier call on this control block ended where this one starts, no opening kernel
QUIET = f"{ONE} T=16 step0=16 progress_valid=1 same_ctrl=1 progress_end=16"


@pytest.fixture(scope="module")
def decide(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("simulate_logic") / "simulate_logic_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "ratinabox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "simulate_logic_host.cpp"), "-o", exe], check=True)

    def run(*rows):
        """one dict per row of facts (values: int, float, or the chunk schedule as a list)"""
        out = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(rows)
        res = []
        for line in out:
            d = {}
            for w in line.split():
                k, v = w.split("=")
                d[k] = ([] if v == "-" else [int(x) for x in v.split(",")]) if k == "sched" else (float(v) if "." in v else int(v))
            res.append(d)
        return res if len(res) > 1 else res[0]
    return run


def _has(d, **kw):
    assert {k: d[k] for k in kw} == kw, d


def test_residency(decide):
    _has(decide(QUIET), form=ONE_KERNEL, strict=0, monotonic=1, open=0, quiet=1, reserve=1, gate=0, launches=2, fork=0, join=0)
    _has(decide(QUIET + " state_published=0"), reserve=1, join=1)   # (the two-wave trajectory kernel)
    _has(decide(QUIET + f" gate_mode={ALWAYS}"), reserve=0, gate=1, launches=3, fork=0, join=0)
    _has(decide(QUIET + f" gate_mode={WHEN_BUSY}"), reserve=0, gate=0, launches=2, fork=0, join=0)
    for mode in (ALWAYS, WHEN_BUSY, RESERVED):
        _has(decide(QUIET + f" idle=0 gate_mode={mode}"), quiet=0, reserve=0, fork=1, gate=1, launches=3, join=1)
    _has(decide(QUIET + " reservable=0"), quiet=1, reserve=0, gate=1, launches=3)
    # not monotonic: no earlier call, another control block, a start behind the last call's end (signed 32-bit distance)
    for facts in (f"{ONE} T=16", QUIET + " same_ctrl=0", QUIET + " step0=10", QUIET + " step0=0x80000011"):
        _has(decide(facts), monotonic=0, quiet=0, reserve=0, gate=1, launches=3)
    _has(decide(QUIET + " step0=5 progress_end=0xfffffff0"), monotonic=1, reserve=1, gate=0)   # (the counter wraps)
    # one stream for both kernels (RIAB_STREAMER_OPT_SIDE_STREAM = 2): no gate could ever return, no event is needed
    _has(decide(QUIET + " side_differs=0 idle=0"), quiet=0, gate=0, fork=0, join=0, launches=2)


def test_mode(decide):
    own = " has_side_own=1"
    _has(decide(f"{ONE} T=256" + own), strict=0)
    _has(decide(f"{ONE} T=257" + own), strict=1)
    _has(decide(f"{ONE} T=257"), strict=0, rc=0)
    _has(decide(f"{TWO} T=257" + own), strict=0)
    _has(decide(f"{TWO} T=257 calibrated=1" + own), strict=1)
    _has(decide(f"{TWO} T=257 step_ns_cfg=100" + own), strict=1)
    _has(decide(f"{TWO} T=256 step_ns_cfg=100" + own), strict=0)
    _has(decide(f"{ONE} T=1024 strict_opt=0" + own), strict=0)
    _has(decide(f"{ONE} strict_opt=1"), rc=EUNSUPPORTED)
    _has(decide(f"{ONE} strict_opt=0 capturing=1"), rc=EUNSUPPORTED)
    for opt in (0, 1, 2):
        _has(decide(f"{ONE} strict_opt={opt} capturing=1" + own), rc=0, strict=1)
    # strict: opening kernel, fork, started gate and join always; whatever `idle` holds
    a, b = decide(QUIET + " strict_opt=1 idle=1" + own, QUIET + " strict_opt=1 idle=0" + own)
    assert a == b
    _has(a, strict=1, open=1, fork=1, quiet=0, reserve=0, gate=1, join=1, launches=4, resync_next=1)
    _has(decide(f"{ONE} T=1024" + own), strict=1, form=ONE_KERNEL, launches=4)
    # after a strict call the next default call opens as well, and counts on from there ...
    _has(decide(QUIET + " resync=1"), strict=0, open=1, fork=1, quiet=0, gate=1, join=1, launches=4, resync_next=0)
    # ... unless a strict call has ever been captured: then every later call opens
    _has(decide(QUIET + " resync=1 captured_once=1"), strict=0, open=1, resync_next=1)
    _has(decide(QUIET), open=0, resync_next=0)


def test_head(decide):
    _has(decide(f"{ONE} T=2048"), form=ONE_KERNEL, head=2048, pure=1, sched=[])
    # 1793 rows behind the head: pieces of 512, 512, 512 and 257 rows, a gate and a kernel each
    _has(decide(f"{ONE} T=2049"), form=HEAD_AND_PIECES, head=256, pure=0, gate=1, launches=1 + 1 + 1 + 2 * 4)
    _has(decide(f"{ONE} T=2049 head_rows=1537"), form=HEAD_AND_PIECES, head=1537, launches=1 + 1 + 1 + 2 * 1)
    _has(decide(f"{ONE} T=3000 head_rows=65535"), form=ONE_KERNEL, head=3000, pure=1)
    _has(decide(f"{ONE} T=100 poll_max=99"), form=CHUNKS, lead=-1, head=0)
    _has(decide(f"{ONE} T=100 poll_max=100"), form=ONE_KERNEL)
    _has(decide(f"{ONE} T=1 poll_max=0"), form=CHUNKS)
    _has(decide(f"{pop(PLACE, 8, 0, 0)} T=16"), form=CHUNKS, sched=[16], gate=0, launches=1 + 2)
    _has(decide("T=16"), form=NONE, launches=1)
    _has(decide(f"{ONE} T=16 forced=1"), form=SERIAL, lead=-1, launches=0)   # (the forced-positions quirk)


def test_lead_and_form(decide):
    d = decide(TWO + " T=33")   # the built-in figures
    _has(d, form=CHUNKS, candidate=0, lead=-1, margin=1.5, step_ns=900.0, sched=[33], launches=1 + 3)
    assert d["row_ns"] == pytest.approx(645.28, abs=0.01)
    # (populations form: the other population's launch is not counted)
    _has(decide(TWO + " T=33 step_ns_cfg=100"), form=POPULATIONS, lead=0, head=33, pure=0, margin=1.5, gate=1, launches=3)
    _has(decide(TWO + " T=33 step_ns_cfg=50000"), form=CHUNKS)
    _has(decide(TWO + " T=33 step_ns_meas=500"), form=CHUNKS, margin=2.0, step_ns=450.0)
    _has(decide(TWO + " T=33 step_ns_meas=300"), form=POPULATIONS, margin=2.0, step_ns=270.0)
    _has(decide(TWO + " T=33 step_ns_meas=300 step_ns_cfg=400"), form=POPULATIONS, margin=1.5, step_ns=400.0)
    _has(decide(TWO + " T=33 lead_mbps_cfg=3000000"), form=POPULATIONS)           # 1398 ns per row
    _has(decide(TWO + " T=33 lead_mbps_meas=3000000"), form=POPULATIONS)
    _has(decide(TWO + " T=33 n_walls=6"), step_ns=1400.0)                           # 250 ns per wall beyond four
    _has(decide(TWO + " T=33 n_walls=3"), step_ns=900.0)
    _has(decide(f"{pop(FF, 100000)} {pop(PLACE, 512)} B=2048 T=33"), candidate=1)   # a feed-forward layer never leads
    _has(decide(f"{pop(PLACE, 512, 1)} {pop(HDC, 4)} B=2048 T=33"), candidate=0, lead=-1, lead_row_bytes=0)
    _has(decide(f"{pop(PLACE, 512, 1)} {pop(HDC, 4)} B=2048 T=33 step_ns_cfg=100"), lead=0, lead_row_bytes=512 * 2048 * 5)
    _has(decide(f"{pop(PLACE, 512)} {pop(GRID, 1024, 0, 0)} {pop(HDC, 600)} B=2048 T=33"), candidate=2)
    _has(decide(f"{pop(BVC, 512, 0, 0)} {pop(BVC, 4, 0, 0)} B=2048 T=33"), candidate=-1, form=CHUNKS)
    # the one blocking read of the stamps: several populations with a candidate, default mode, not yet made, nothing configured,
    # the earlier call on this stream
    _has(decide(TWO + " T=33"), calibration_due=1)
    for off in ("calibrated=1", "step_ns_cfg=100", "same_stream=0", "strict_opt=1 has_side_own=1", "poll_max=10"):
        _has(decide(TWO + " T=33 " + off), calibration_due=0)
    _has(decide(ONE), calibration_due=0)


def test_chunk_ramp(decide):
    no_lead = pop(BVC, 8, 0, 0)
    _has(decide(f"{no_lead} T=1024"), sched=[16, 28, 44, 64, 96, 128, 128, 128, 128, 128, 136], launches=1 + 2 * 11)
    _has(decide(f"{no_lead} T=64 periodic=1"), sched=[16, 16, 32])
    _has(decide(f"{no_lead} T=20"), sched=[20])
    _has(decide(f"{no_lead} T=400 n_walls=3"), sched=[16, 16, 20, 24, 32, 40, 48, 64, 80, 60])
    lengths = list(range(1, 700)) + [1023, 1024, 1025, 2048, 4097, 65535]
    rooms = ("", "periodic=1", "polygon=1", "hole_mask=16")
    res = decide(*(f"{no_lead} T={T} {room}" for room in rooms for T in lengths))
    for (room, T), d in zip(itertools.product(rooms, lengths), res):
        s = d["sched"]
        assert sum(s) == T and min(s) >= 1 and (len(s) == 1 or s[-1] >= 32), (room, T, s)
        assert d["launches"] == 1 + 2 * len(s)


def test_timing(decide):
    own = " has_side_own=1"
    # no lead, or a lead that is not the only kernel: pairs of events
    _has(decide(TWO + " T=33 step_ns_cfg=100 timed_pop=0"), timing=1, pairs_needed=2 * (1 + 1), events=0)
    _has(decide(TWO + " T=1025 step_ns_cfg=100 timed_pop=1 strict_opt=0"), timing=1, pairs_needed=2 * (1 + 2))
    _has(decide(f"{ONE} T=2049 timed_pop=0"), timing=1, pairs_needed=2 * (1 + 3))
    _has(decide(TWO + " T=1024 timed_pop=1"), form=CHUNKS, timing=1, pairs_needed=2 * 11)
    _has(decide(TWO + " T=1024 timed_pop=2"), timing=0, pairs_needed=0)
    _has(decide(TWO + " T=1024"), timing=0, pairs_needed=0)
    # a strict call creates nothing: short of events it is not timed, and that is no error
    _has(decide(TWO + " T=1024 timed_pop=1 strict_opt=1 pairs=21" + own), rc=0, strict=1, timing=0, pairs_needed=0)
    _has(decide(TWO + " T=1024 timed_pop=1 strict_opt=1 pairs=22" + own), rc=0, strict=1, timing=1, pairs_needed=22)
    _has(decide(f"{ONE} timed_pop=0 timing_mode=1 strict_opt=1 pairs=0" + own), timing=0, events=0, stamps=1)
    _has(decide(f"{ONE} timed_pop=0 timing_mode=1 strict_opt=1 pairs=2" + own), timing=1, events=1, stamps=0)
    _has(decide(f"{ONE} timed_pop=0 capturing=1 pairs=64" + own), timing=0)   # (no timing events inside a capture)
    # the one kernel: the device's stamps unless HIP events are asked for
    _has(decide(f"{ONE} timed_pop=0"), timing=1, pairs_needed=0, events=0, stamps=1)
    _has(decide(f"{ONE} timed_pop=0 timing_mode=1"), timing=1, pairs_needed=2, events=1, stamps=0)
    _has(decide(f"{ONE} timing_mode=1"), timing=0, events=0, stamps=1)
    _has(decide(f"{ONE} T=2049 timed_pop=0 timing_mode=1"), pure=0, events=0, stamps=1)


# Calls that test_gpu_fused.test_real_calls_take_the_decisions_of_the_logic_header really makes (an Agent of 256 agents: its
# streamer has been warmed up, every call follows a synchronise and continues the earlier call's control block): facts ->
# (form, strict, launches).  The strict call of 257 steps leaves `resync` set for the calls behind it.
_WARM = "B=256 has_side_own=1 progress_valid=1 same_ctrl=1"
REAL_CALLS_ONE = [(8, "", (ONE_KERNEL, 0, 2)), (256, "", (ONE_KERNEL, 0, 2)), (257, "", (ONE_KERNEL, 1, 4)),
                  (2048, "resync=1", (ONE_KERNEL, 1, 4)), (2049, "resync=1", (HEAD_AND_PIECES, 1, 2 + 1 + 1 + 2 * 4))]
# PlaceCells 8 + HeadDirectionCells 4, 33 steps: 8 KB per row is 1.3 ns of stores — no configured step is that short (chunks:
# trajectory, one gate, two kernels); a configured store rate of 1 GB/s makes it 8 us (populations: trajectory, gate, lead)
REAL_CALLS_TWO = [("step_ns_cfg=100", (CHUNKS, 0, 4)), ("step_ns_cfg=50000", (CHUNKS, 0, 4)),
                  ("step_ns_cfg=100 lead_mbps_cfg=1000", (POPULATIONS, 0, 3))]


def test_the_calls_the_gpu_test_makes(decide):
    for T, more, (form, strict, launches) in REAL_CALLS_ONE:
        _has(decide(f"{ONE} {_WARM} T={T} {more}"), form=form, strict=strict, launches=launches)
    for more, (form, strict, launches) in REAL_CALLS_TWO:
        _has(decide(f"{pop(PLACE, 8)} {pop(HDC, 4)} {_WARM} T=33 {more}"), form=form, strict=strict, launches=launches)


def test_join(decide):
    cases = list(itertools.product((0, 1), repeat=5))
    res = decide(*(QUIET + f" state_published={sp} fail={fail} idle={idle} resync={opn} side_differs={side}"
                   for sp, fail, idle, opn, side in cases))
    for (sp, fail, idle, opn, side), d in zip(cases, res):
        assert d["open"] == opn and d["join"] == int((not sp or fail or not idle or opn) and side), (sp, fail, idle, opn, side)
        assert d["fork"] == int((not idle or opn) and side)
