"""examples/value_learning_example.py with the whole loop inside a step plan: 4096 agents wander in one room each, every
one of them is rewarded when it stands in the goal in the middle, and ONE ValueNeuron — fed by all of them at once —
learns the value of a position as a weighted sum of 1024 PlaceCells.  `env.make_step_plan()` records the agent, the
PlaceCells and the LEARNING ValueNeuron once; every `plan.step(n)` then runs n times, in one native call,

    env.step(None); PCs.update(); VN.learn(env.get_reward()); done = env.terminal; VN.reset(lanes=done); env.reset(mask=done)

— the loop of the other example, in its order ("learn, then reset"): the reward goes from the task to the learner on the
device, and finished episodes reset their agents' traces before the task teleports them.

    python examples/value_learning_plan_example.py [steps]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ratinabox_amd as riab  # noqa: E402
from ratinabox_amd.contribs.TaskEnvironment import SpatialGoalEnvironment  # noqa: E402
from ratinabox_amd.contribs.ValueNeuron import ValueNeuron  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
np.random.seed(0)
goal, corner = np.array([[0.5, 0.5]]), np.array([[0.05, 0.05]])

env = SpatialGoalEnvironment(possible_goal_positions=goal.tolist(), goalkws={"goal_radius": 0.1},
                             goalcachekws=dict(reset_n_goals=1), teleport_on_reset=True, dt=0.05, seed=1)
Ag = riab.Agent(env, {"n_agents": 4096, "dt": 0.05, "speed_mean": 0.2, "save_history": False})
env.add_agents(Ag)
PCs = riab.PlaceCells(Ag, {"n": 1024, "widths": 0.1, "save_history": False})
# (a linear read-out, so that the learner can start from "no value anywhere": a relu at zero has no gradient)
VN = ValueNeuron(Ag, {"input_layers": [PCs], "tau": 1.0, "eta": 0.01, "activation_function": {"activation": "linear"},
                      "save_history": False})
w = VN.inputs[PCs.name]
w["w"] = np.zeros_like(w["w"])


def value_at(pos):
    return float(VN.get_state(evaluate_at=None, pos=pos)[0, 0])


print(f"before: value at the goal {value_at(goal):.4f}, in the corner {value_at(corner):.4f}")
plan = env.make_step_plan(auto_reset=True)   # random exploration; the ValueNeuron learns from the task's reward
torch.cuda.synchronize()
t0 = time.perf_counter()
left = steps
while left > 0:
    n = min(left, 100)
    plan.step(n)                              # n closed-loop steps, learning included, in one native call
    left -= n
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f"{steps} steps x 4096 agents in {dt:.2f} s ({dt / steps * 1e6:.0f} us per step, loop and environment included)")
print(f"after:  value at the goal {value_at(goal):.4f}, in the corner {value_at(corner):.4f}")
assert value_at(goal) > value_at(corner)
