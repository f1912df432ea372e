"""Replays on the device: the reference's usage of contribs.SubAgent.ReplayAgent — a lead Agent, a ReplayAgent slaved to
it, PlaceCells on the replaying position — for one agent, then 1024 agents at once.

    python examples/replay_example.py [steps]

Outside a replay a lane starts one with probability replay_freq x dt per step, so replays start at `replay_freq` per
second of time spent outside; a replay lasts a Rayleigh draw of scale `replay_duration`, floored at half of it (mean
about 1.28 x replay_duration), rounded up to whole steps.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ratinabox_amd as riab  # noqa: E402
from ratinabox_amd.contribs.SubAgent import ReplayAgent  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
np.random.seed(0)
DT = 0.01


def expected_duration(scale):
    """E[max(Rayleigh(scale), scale / 2)]"""
    r = np.random.RandomState(1).rayleigh(scale, 200000)
    return float(np.maximum(r, scale / 2).mean())


def report(tag, flags, rep, dt):
    """flags (T, B) bool: fraction of the time in replay, replays per second outside, their mean length"""
    flags = flags.reshape(len(flags), -1)
    starts = int((flags[1:] & ~flags[:-1]).sum() + flags[0].sum())
    ends = int((~flags[1:] & flags[:-1]).sum())
    outside = float((~flags).sum()) * dt
    length = float(flags.sum()) * dt / max(starts, 1)
    print(f"{tag}: {100 * flags.mean():.1f} % of the time in replay; {starts} replays started ({ends} ended), "
          f"{starts / outside:.2f} per second outside replay (replay_freq {rep.replay_freq}); mean length {length:.3f} s "
          f"(expected {expected_duration(rep.mean_replay_duration) + dt / 2:.3f} s for replay_duration "
          f"{rep.mean_replay_duration}); {rep.replay_diagnostics}")
    return starts


# ---- one agent: five minutes of its life -------------------------------------------------------------------------------
Env = riab.Environment()
Lead = riab.Agent(Env, {"dt": DT})
Rep = ReplayAgent(Lead)
PCs = riab.PlaceCells(Rep, {"n": 32, "widths": 0.1, "wall_geometry": "euclidean"})
for _ in range(30000):
    Lead.update()
    Rep.update()
    PCs.update()
flags = np.asarray(Rep.history["replay"])
jump = np.linalg.norm(np.asarray(Rep.history["pos"]) - np.asarray(Lead.history["pos"]), axis=-1)
n = report("one agent, 300 s", flags, Rep, DT)
print(f"    distance from the lead: {jump[flags].mean():.2f} m during replays, {jump[~flags].max():.2g} m outside them")
assert n > 30 and not jump[~flags].any() and jump[flags].mean() > 0.1

# ---- 1024 agents ---------------------------------------------------------------------------------------------------------
B = 1024
Lead = riab.Agent(riab.Environment(), {"n_agents": B, "dt": DT, "save_history": False})
Rep = ReplayAgent(Lead)
PCs = riab.PlaceCells(Rep, {"n": 256, "widths": 0.1, "wall_geometry": "euclidean", "save_history": False})
for _ in range(10):
    Lead.update(); Rep.update(); PCs.update()
torch.cuda.synchronize()
Rep.reset_history()
t0 = time.perf_counter()
for _ in range(steps):
    Lead.update()
    Rep.update()
    PCs.update()
torch.cuda.synchronize()
wall = time.perf_counter() - t0
report(f"{B} agents, {steps * DT:.0f} s", np.asarray(Rep.history["replay"]), Rep, DT)
print(f"    {steps} steps x {B} agents x {PCs.n} place cells on the replaying position in {wall:.2f} s "
      f"({wall / steps * 1e6:.0f} us per step), at most {Rep.replay_steps_max} sham steps per update")
assert np.asarray(Rep.pos).shape == (B, 2)
