"""No-GPU checks of the built gfx950 code objects (libriab_hip.so, as the package builds it) for what no test on the
device can see: the one-world ticket's drain and which kernels have a stack frame."""
import os
import re
import shutil
import subprocess

import pytest

LLVM_BIN = "/opt/rocm/llvm/bin"

RET_ADD = re.compile(r"^(global|flat)_atomic_add(_u32)?\s.*\bsc0\b")  # a returning atomic add
STORE = re.compile(r"^(global|flat|scratch|buffer)_(store|atomic)")
TERMINAL = re.compile(r"^global_store_byte\s.*\bsc1\b")  # phase A's last write-through store: the `terminal` column
# Every kernel with a stack frame, and its size in bytes.  The two step1 instantiations are the ones launch_step1_impl
# refuses (a frame needs scratch set up per dispatch); the float64 helper-wave motion kernels carry a
# small one.  A kernel that gains a frame, or a frame that grows, fails here.
FRAMES = {"_ZN4riab17step1_task_kernelILi1ELi11ELin1EEE": 352, "_ZN4riab17step1_task_kernelILi1ELi15ELin1EEE": 352,
          "_ZN4riab17agent_step_kernelIdLi0ELb1ELb0EEE": 36, "_ZN4riab17agent_step_kernelIdLi0ELb1ELb1EEE": 36}


def _tool(name):
    path = os.path.join(LLVM_BIN, name)
    return path if os.path.exists(path) else shutil.which(name)


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    objdump, readelf = _tool("llvm-objdump"), _tool("llvm-readelf")
    if not objdump or not readelf:
        pytest.skip("llvm-objdump / llvm-readelf not found")
    from ratinabox_amd import _build
    tmp = tmp_path_factory.mktemp("isa")
    lib = shutil.copy(_build.build(), tmp / "libriab_hip.so")
    subprocess.run([objdump, "--offloading", str(lib)], cwd=tmp, check=True, capture_output=True)
    cos = sorted(str(p) for p in tmp.iterdir() if p.name.endswith("gfx950"))  # (one per translation unit)
    assert cos, "no gfx950 code object in the library"
    disasm = subprocess.run([objdump, "-d", "--mcpu=gfx950", *cos], check=True, capture_output=True, text=True).stdout
    notes = subprocess.run([readelf, "--notes", *cos], check=True, capture_output=True, text=True).stdout
    return disasm, notes


def _kernels(disasm):
    """symbol -> its instructions, operands kept, encodings and comments dropped"""
    out, cur = {}, None
    for line in disasm.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        s = line.split("//")[0].strip()
        if cur is not None and s:
            cur.append(s)
    return out


def _one_world(name):
    m = re.match(r"_ZN4riab17step1_task_kernelILi\d+ELi(\d+)E", name)
    return (m is not None and int(m.group(1)) & 8) or "task_world_step_kernel" in name or "motion_world_kernel" in name


def _tickets(ins):
    """(wait, stores between it and the ticket, ticket) for each ticket: the first returning atomic add behind phase A's
    write-through `terminal` store.  `wait` is the instruction in front of the last s_barrier between the two (a
    one-wave workgroup has none: then the last s_waitcnt between them)."""
    out = []
    for i, s in enumerate(ins):
        if not TERMINAL.match(s):
            continue
        t = next((j for j in range(i + 1, len(ins)) if RET_ADD.match(ins[j])), None)
        if t is None:
            continue
        bars = [b for b in range(i, t) if ins[b] == "s_barrier"]
        w = bars[-1] - 1 if bars else max([k for k in range(i, t) if ins[k].startswith("s_waitcnt")] or [i])
        out.append((ins[w], [x for x in ins[w + 1:t] if STORE.match(x)], ins[t]))
    return out


def test_one_world_ticket_is_taken_after_phase_a_stores_drain(code_object):
    ks = _kernels(code_object[0])
    world = sorted(k for k in ks if _one_world(k))
    assert any("task_world_step_kernel" in k for k in world) and any("motion_world_kernel" in k for k in world)
    assert sum("step1_task_kernel" in k for k in world) >= 8, world
    for k in world:
        t = _tickets(ks[k])
        assert len(t) == 1, (k, t)
        wait, stores, ticket = t[0]
        assert re.match(r"^s_waitcnt\b.*\bvmcnt\(0\)", wait), f"{k}: the ticket ({ticket}) is taken behind `{wait}`"
        assert not stores, (k, stores)


def test_only_the_known_kernels_have_a_stack_frame(code_object):
    frames = {}
    for m in re.finditer(r"^ {4}\.name:\s+(\S+)\n(.*?)^ {4}\.symbol:", code_object[1], re.S | re.M):
        f = re.search(r"\.private_segment_fixed_size:\s+(\d+)", m.group(2))
        frames[m.group(1)] = int(f.group(1)) if f else 0
    assert len(frames) > 100
    framed = {next((p for p in FRAMES if k.startswith(p)), k): v for k, v in frames.items() if v}
    assert framed == FRAMES and sum(1 for v in frames.values() if v) == len(FRAMES), framed
