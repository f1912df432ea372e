"""Guard bands around the kernels whose contract is NOT "every element of the output, once": the SubAgent kernels, the rate
maps, the stand-alone geometry queries and the rate ring of a population that keeps no history (tests/guard_arena.py;
tests/test_guard_arena_cpu.py shows that the checker finds what is planted, in its `written=` and `inplace=` modes too).

tests/test_gpu_guard_bands.py pins where every population kernel writes.  The kernels here keep state that is updated in
place, ring slots, per-lane tables that are written up to a lane's own count, and rows that a wave leaves alone once its
last lane is done: a store from a lane b >= B of the last wave, a ring slot off by one or a `future` row k + 2 lands in
allocator slack or in a row that is overwritten later, and no value test reads either.  Every buffer a kernel is handed
here — inputs too, so that a stray READ lands in memory the test owns — is a view in the middle of a canary-filled
allocation, every case runs with both canaries, and `check` asserts, by the buffer's contract:

    fully written        both guards intact, no interior element holds the canary, the same bits with both canaries
    written=mask         ... and the elements the contract leaves alone still hold the canary, bit for bit
    inplace=True         state the test pre-filled: the guards, and the same bits with both canaries
    inputs               inplace=True with other=<what went in>: not a bit changed

The interior is compared in the same test with the float64 oracle the suite already has, under the tolerance of the
existing test that is named beside each assertion (none new).  Every kernel is called through its raw export
(`ratinabox_amd._lib`), so the test owns every buffer; the classes are used for the environment and motion structs only
(the ring: `Neurons._reserve_rows_at` / `_reserve_rows` patched test-side to hand back an arena view).
(B, n_agents) is (4, 3): one wave with 60 idle lanes; (68, 65): a second wave with 4 live lanes; (132, 130).

Padding poison (NaN and 3e38 in the inputs of the lanes >= n_agents must change no bit of a real lane and no counter) is
asserted for riab_theta_sequence_step, riab_shift_agent_position, riab_history_bin_index and riab_history_rate_map, and NOT
for the rollout, replay and dumb kernels: agent_step_body takes wave-uniform decisions, so a lane's bits may
depend on its wave by design, and those kernels are fed finite state only."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import riab_oracle as orc
from tests import guard_arena as ga
from tests import ratemap_oracle as rmo
from tests import replay_oracle as rpo
from tests import subagent_oracle as sao
from tests.test_gpu_replay import DT as REPLAY_DT, FLOOR, lead_path, sham_state_dict

pytestmark = pytest.mark.gpu

SHAPES = [(4, 3), (68, 65), (132, 130)]
SHAPE_IDS = [f"B{B}-n{n}" for B, n in SHAPES]
POISON = (float("nan"), 3e38)
BOX_WALL = [[0.5, 0.0], [0.5, 0.5]]          # the walled box of tests/test_gpu_subagent.py and tests/test_gpu_replay.py


def box(riab, kind):
    """the room of those two files: "wall" (the box with one wall) or "periodic" """
    env = riab.Environment({"boundary_conditions": "periodic"} if kind == "periodic" else {})
    if kind == "wall":
        env.add_wall(np.array(BOX_WALL))
    return env


def oracle_box(kind):
    return orc.EnvSpec(boundary_conditions="periodic" if kind == "periodic" else "solid", walls=[BOX_WALL] if kind == "wall" else [])


@pytest.fixture(scope="module")
def riab():
    assert torch.cuda.is_available(), "these tests need the GPU"
    import ratinabox_amd
    return ratinabox_amd


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def put(arena, a, dtype=None):
    """`a` in an arena view on the device: an input, or state the kernel updates in place"""
    a = np.ascontiguousarray(a, dtype=dtype)
    t = torch.from_numpy(a)
    v = arena.view(a.shape, t.dtype, "cuda")
    v.copy_(t)
    return v


def unchanged(arena, view, a):
    """an input after the launch: both guards intact and not a bit of it changed"""
    if view is None:
        return
    arena.check(view, inplace=True, other=np.ascontiguousarray(a))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}")


def call(L, name, *args):
    rc = getattr(L.lib, name)(*args)
    assert rc == 0, (name, L.strerror(rc))
    torch.cuda.synchronize()


def lead_rows(B, rs, speed=None, dist=None):
    """a lead's float64 state [12][B]: every lane, the padding lanes included, holds an ordinary agent"""
    s = np.zeros((12, B))
    s[0:2] = rs.uniform(0.1, 0.9, (2, B))
    ang, hd = rs.uniform(0, 2 * np.pi, B), rs.uniform(0, 2 * np.pi, B)
    v = rs.uniform(0.02, 0.2, B) if speed is None else speed
    s[2:4] = v * np.stack((np.cos(ang), np.sin(ang)))
    s[4] = rs.normal(0, 1.0, B)
    s[5:7] = s[2:4]
    s[8:10] = np.stack((np.cos(hd), np.sin(hd)))
    s[10] = rs.uniform(0.0, 1.0, B) if dist is None else dist
    s[11] = 0.1
    return s


def lead_dict(s):
    return dict(pos=s[0:2].T.copy(), velocity=s[2:4].T.copy(), rotational_velocity=s[4].copy(), distance_travelled=s[10].copy())


def poisoned(a, n, value):
    """`a` [...][B] with the lanes >= n set to `value`"""
    a = np.array(a, copy=True)
    a[..., n:] = value
    return a


# ---------------------------------------------------------------------------------------------------------------------
# riab_shift_agent_position
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n", SHAPES, ids=SHAPE_IDS)
def test_shift_agent_position(riab, B, n):
    """pos_out [2][B] fully written and, bit for bit, the float64 expression (tests/test_gpu_subagent.py test_shift_agent
    allows 1e-15; every operation is rounded on its own, so the bits are NumPy's); NaN / 3e38 in the lanes >= n of the
    lead's state change no bit of a lane < n."""
    L = riab._lib
    lead = lead_rows(B, np.random.RandomState(B))
    for shift in (0.03, -0.03):
        want = sao.shift_position(lead[0:2].T, lead[8:10].T, shift).T
        first = None
        for canary in ga.CANARIES:
            arena = ga.GuardArena(canary)
            lead_t, out = put(arena, lead), arena.view((2, B), torch.float64, "cuda")
            call(L, "riab_shift_agent_position", L.ptr(lead_t), B, shift, L.ptr(out), L.current_stream())
            first = arena.check(out, other=first)
            unchanged(arena, lead_t, lead)
        np.testing.assert_array_equal(bits(first), bits(want))
        for value in POISON:
            bad = poisoned(lead, n, value)
            arena = ga.GuardArena("nan")
            lead_t, out = put(arena, bad), arena.view((2, B), torch.float64, "cuda")
            call(L, "riab_shift_agent_position", L.ptr(lead_t), B, shift, L.ptr(out), L.current_stream())
            got = arena.check(out)
            np.testing.assert_array_equal(bits(got[:, :n]), bits(first[:, :n]))


@pytest.mark.parametrize("canary", ga.CANARIES)
def test_control_a_wider_launch_lands_in_the_back_guard(riab, canary):
    """Positive control of the fully-written mode, no kernel changed: riab_shift_agent_position with B + 4 lanes on a
    pos_out declared for B = 4.  Row y of the wider launch starts at element B + 4, so its lanes B - 4 .. B + 3 land on
    the 8 elements behind the view: (2, 0, 0..3) and (3, 0, 0..3) of a view laid out [2][1][B]."""
    L, B = riab._lib, 4
    lead = lead_rows(B + 4, np.random.RandomState(1))
    arena = ga.GuardArena(canary)
    lead_t, out = put(arena, lead), arena.view((2, 1, B), torch.float64, "cuda")
    call(L, "riab_shift_agent_position", L.ptr(lead_t), B + 4, 0.03, L.ptr(out), L.current_stream())
    with pytest.raises(ga.GuardError) as e:
        arena.check(out)
    assert e.value.kind == "back guard" and e.value.count == 8
    assert e.value.first == (2, 0, 0) and e.value.last == (3, 0, 3)
    want = sao.shift_position(lead[0:2].T, lead[8:10].T, 0.03).T           # [2][B + 4]
    base = arena.base(out)
    end = (out.data_ptr() - base.data_ptr()) // 8 + out.numel()          # offset of the first element behind the view
    behind = base[end:end + 4].cpu().numpy()
    np.testing.assert_array_equal(behind, want[1, B - 4:B])                # (2, 0, 0..3): y of the lanes B - 4 .. B - 1


# ---------------------------------------------------------------------------------------------------------------------
# riab_theta_sequence_rollout
# ---------------------------------------------------------------------------------------------------------------------
K_ROLL, DT_FORWARD, FORWARD_DISTANCE, DT_LEAD = 6, 0.05, 0.018, 0.01


def rollout_inputs(B):
    """The lead's state for a rollout whose lanes need 0 .. K steps and more: speeds log-spaced over 0.02 .. 1.5 m/s (a lane
    covers FORWARD_DISTANCE in about 0.6 / speed steps), and one lane per wave whose distance travelled is 1e16, where
    distance + FORWARD_DISTANCE is the distance itself: it is there before its first step."""
    rs = np.random.RandomState(900 + B)
    speed = np.exp(rs.permutation(np.linspace(np.log(0.02), np.log(1.5), B)))
    if B == 4:
        speed = np.array([0.3, 1.2, 0.005, 0.15])
    dist = rs.uniform(0.0, 1.0, B)
    dist[(np.arange(B) % 64) == (0 if B == 4 else 5)] = 1e16
    lead = lead_rows(B, rs, speed=speed, dist=dist)
    fwd0 = lead_rows(B, rs)                                  # what the ForwardSequenceAgent's rows hold before the call
    z = rs.standard_normal((K_ROLL, 2, B))
    return lead, fwd0, z


def rollout_oracle(B, lead, z):
    o = sao.ThetaSequenceOracle(oracle_box("wall"), B, DT_LEAD, 0.08, v_sequence=2.0)
    o.K, o.dt_forward, o.forward_distance = K_ROLL, DT_FORWARD, FORWARD_DISTANCE
    o.rollout(lead_dict(lead), z)
    count = o.rollouts[-1]["count"]
    saturated = (count == K_ROLL) & (o.forward_final["distance_travelled"] < lead[10] + FORWARD_DISTANCE)
    return o, count, saturated


def rollout_masks(count, B):
    """written-masks of future [K + 1][3][B] (entries 0 .. count[b]) and z_out [K][2][B] (the rows below the last step of
    the lane's 64-lane wave: a wave steps while one of its lanes is short of its target)"""
    k = np.arange(K_ROLL + 1)[:, None]
    future = np.broadcast_to((k <= count[None, :])[:, None, :], (K_ROLL + 1, 3, B)).copy()
    last = np.array([count[w * 64:(w + 1) * 64].max() for w in range((B + 63) // 64)])
    z_out = np.broadcast_to((k[:K_ROLL] < last[np.arange(B) // 64][None, :])[:, None, :], (K_ROLL, 2, B)).copy()
    return future, z_out


def agent_steps(L, env, m, B, id0, start, n, z=None, seed=0, step0=0):
    """`n` calls of riab_agent_step(T = 1) from `start` [12][B] (device), with the normals z [K][2][B] (device) or the
    Philox stream (seed; step0 + k): the states after each call, (n + 1, 12, B)"""
    st = start.clone()
    out = [st.cpu().numpy()]
    for k in range(n):
        call(L, "riab_agent_step", env, m, L.ptr(st), B, id0, None, L.ptr(z[k]) if z is not None else None, None, None, None,
             seed, step0 + k, 1, None, None, L.current_stream())
        out.append(st.cpu().numpy())
    return np.stack(out)


class Rollout:
    """One riab_theta_sequence_rollout with every buffer in `arena`."""

    def __init__(self, riab, B, n, canary, philox):
        L = self.L = riab._lib
        self.B, self.n, self.philox = B, n, philox
        self.lead, self.fwd0, self.z = rollout_inputs(B)
        np.random.seed(5)
        self.env_obj = box(riab, "wall")
        self.fwd = riab.Agent(self.env_obj, {"n_agents": n, "dt": DT_LEAD})
        assert self.fwd._Bp == B
        self.env, self._walls = self.env_obj.device_tables(self.fwd._device)
        self.m = self.fwd._motion(DT_FORWARD, False, 1, {})
        self.seed, self.step0, self.id0 = int(self.fwd.rng_seed), 7 * K_ROLL, 4096
        a = self.arena = ga.GuardArena(canary)
        self.lead_t, self.state, self.z_in = put(a, self.lead), put(a, self.fwd0), put(a, self.z)
        self.z_out = a.view((K_ROLL, 2, B), torch.float64, "cuda")
        self.future = a.view((K_ROLL + 1, 3, B), torch.float64, "cuda")
        self.count = a.view((B,), torch.int32, "cuda")
        self.diag = put(a, np.zeros(4, dtype=np.int32))
        call(L, "riab_theta_sequence_rollout", self.env, self.m, L.ptr(self.lead_t), L.ptr(self.state), B, n, self.id0,
             None if philox else L.ptr(self.z_in), L.ptr(self.z_out), self.seed, self.step0, K_ROLL, FORWARD_DISTANCE,
             L.ptr(self.future), L.ptr(self.count), None, L.ptr(self.diag), L.current_stream())

    def start(self):
        """what the rollout starts from: the ForwardSequenceAgent's rows with the lead's position, velocity, rotational
        velocity and distance (tests/test_gpu_subagent.py rollout_start)"""
        s = self.fwd0.copy()
        for r in (0, 1, 2, 3, 4, 10):
            s[r] = self.lead[r]
        return s


@pytest.mark.parametrize("philox", [False, True], ids=["explicit", "philox"])
@pytest.mark.parametrize("B,n", SHAPES, ids=SHAPE_IDS)
def test_theta_sequence_rollout(riab, B, n, philox):
    """forward_state [12][B] in place; future [K + 1][3][B] written in the entries 0 .. count[b] of each lane and in no
    other; z_out [K][2][B] in the rows below its wave's last step and in no other; count [B] fully written; lead_state and
    z_in not a bit changed.  The interior as tests/test_gpu_subagent.py has it: table, counts and final state bit for bit
    what riab_agent_step(T = 1) gives from the same start (test_rollout_is_the_motion_kernel); the counts the oracle's
    (run_sweep: "steps per lane, kernel against oracle"); the table against the oracle's own rollout within 4 x the
    deviation of riab_agent_step from oracle.agent_step over the same steps, floor 1e-12 (check_sweep); Philox normals
    against oracle.motion_normals to test_philox_rollouts' rtol 1e-5, atol 2e-5."""
    L = riab._lib
    lead, _fwd0, z = rollout_inputs(B)
    o = count_o = sat_o = None
    if not philox:                     # (the oracle first, on the CPU: the case is what the docstring says it is)
        o, count_o, sat_o = rollout_oracle(B, lead, z)
        seen = set(count_o[:64].tolist())
        # one wave spans 0 .. K steps and holds lanes that ran out (B = 4: four lanes, four different counts, 0 among them)
        assert (seen == set(range(K_ROLL + 1)) and sat_o[:64].any()) if B > 4 else (0 in seen and len(seen) == 4), sorted(seen)
    got = {}
    for canary in ga.CANARIES:
        r = Rollout(riab, B, n, canary, philox)
        a = r.arena
        count = a.check(r.count, other=got.get("count"))
        assert count.min() >= 0 and count.max() <= K_ROLL
        m_future, m_z = rollout_masks(count, B)
        future = a.check(r.future, written=m_future, other=got.get("future"))
        z_out = a.check(r.z_out, written=m_z, other=got.get("z_out"))
        state = a.check(r.state, inplace=True, other=got.get("state"))
        diag = a.check(r.diag, inplace=True, other=got.get("diag"))
        unchanged(a, r.lead_t, r.lead)
        unchanged(a, r.z_in, r.z)
        got = dict(count=count, future=future, z_out=z_out, state=state, diag=diag)
    count, future, z_out = got["count"], got["future"], got["z_out"]
    m_future, m_z = rollout_masks(count, B)
    ids = r.id0 + np.arange(B)
    if philox:
        for k in range(K_ROLL):
            w = m_z[k, 0]
            z_rot, z_spd, _z2, _z3 = orc.motion_normals(r.seed, r.step0 + k, ids)
            np.testing.assert_allclose(z_out[k, 0][w], z_rot[w], rtol=1e-5, atol=2e-5)
            np.testing.assert_allclose(z_out[k, 1][w], z_spd[w], rtol=1e-5, atol=2e-5)
        o, count_o, sat_o = rollout_oracle(B, lead, np.where(m_z, z_out, 0.0))
    else:
        np.testing.assert_array_equal(bits(z_out[m_z]), bits(z[m_z]))
    np.testing.assert_array_equal(count, count_o, err_msg="steps per lane, kernel against oracle")
    assert got["diag"].tolist() == [0, 0, int(sat_o[:n].sum()), 0]
    # ---- bit for bit the motion kernel
    ref = agent_steps(L, r.env, r.m, B, r.id0, dev(r.start()), int(count.max()), None if philox else dev(z), r.seed, r.step0)
    dev_motion = 0.0
    for b in range(B):
        c = int(count[b])
        for row, s in ((0, L.S_DIST), (1, L.S_POS_X), (2, L.S_POS_Y)):
            np.testing.assert_array_equal(bits(future[:c + 1, row, b]), bits(ref[:c + 1, s, b]), err_msg=f"lane {b} row {row}")
        np.testing.assert_array_equal(bits(got["state"][:, b]), bits(ref[c, :, b]), err_msg=f"final state of lane {b}")
        d, p = o.future[b]
        assert len(d) == c + 1
        dev_motion = max(dev_motion, np.abs(ref[:c + 1, L.S_DIST, b] - d).max(), np.abs(ref[:c + 1, L.S_POS_X, b] - p[:, 0]).max(),
                         np.abs(ref[:c + 1, L.S_POS_Y, b] - p[:, 1]).max())
    bound = max(4 * dev_motion, FLOOR)
    err = max(max(np.abs(future[:count[b] + 1, 0, b] - o.future[b][0]).max(),
                  np.abs(future[:count[b] + 1, 1:3, b] - o.future[b][1]).max()) for b in range(B))
    print(f"[rollout B={B} {'philox' if philox else 'explicit'}] counts {np.bincount(count, minlength=K_ROLL + 1).tolist()}, "
          f"saturated {int(sat_o.sum())}; riab_agent_step against oracle.agent_step {dev_motion:.3g}; table against the oracle "
          f"{err:.3g} (bound {bound:.3g})")
    assert err <= bound


@pytest.mark.parametrize("canary", ga.CANARIES)
def test_control_a_future_entry_the_mask_does_not_claim(riab, canary):
    """Positive control of the written-mask mode, no kernel changed: the rollout's `future` checked against a mask that
    claims one entry fewer than count[b] for one lane must fail as "written where the contract says untouched" and name
    that entry's three rows."""
    B, n = 68, 65
    r = Rollout(riab, B, n, canary, False)
    count = r.arena.check(r.count)
    m_future, _ = rollout_masks(count, B)
    r.arena.check(r.future, written=m_future)                       # the true contract holds
    lane = int(np.nonzero(count >= 2)[0][-1])
    c = int(count[lane])
    m_future[c, :, lane] = False
    with pytest.raises(ga.GuardError) as e:
        r.arena.check(r.future, written=m_future)
    assert e.value.kind == ga.UNTOUCHED and e.value.count == 3
    assert e.value.first == (c, 0, lane) and e.value.last == (c, 2, lane)


# ---------------------------------------------------------------------------------------------------------------------
# riab_theta_sequence_step
# ---------------------------------------------------------------------------------------------------------------------
RING = 8                 # capacity = lookback
V_SEQUENCE = 2.0
D_HALF = (0.5 / 2) * (1 / 10.0) * V_SEQUENCE        # (theta_frac / 2) T_theta v_sequence = 0.05, as the oracle computes it
STEP_CASES = [("none", 0, 0.1), ("none", 9, 0.9), ("behind", 0, 0.4), ("behind", 7, 0.3), ("behind", 8, 0.4), ("behind", 9, 0.45),
              ("ahead", 9, 0.52), ("ahead", 8, 0.55), ("ahead", 7, 0.58)]


def step_inputs(B, n_records, periodic, ahead):
    """The lead's state and the records of its `n_records` earlier steps, (n_records, B) distances and (n_records, B, 2)
    positions.  Even lanes are short of d_half (their position is the lead's), the others beyond it (they interpolate
    the ring); every fifth lane's path is stretched by 8, which puts its point further than d_half from the lead (NaN,
    counted); in the periodic box every seventh lane sits by the edge, so its path wraps."""
    rs = np.random.RandomState(100 * n_records + B + 7 * periodic)
    lane = np.arange(B)
    dist = np.where(lane % 2 == 0, rs.uniform(0.0, 0.04, B), rs.uniform(0.5, 1.0, B))
    lead = lead_rows(B, rs, dist=dist)
    if ahead:                                            # the lead the rollout started from: the table is its future
        lead = rollout_inputs(B)[0]
    if periodic:
        lead[0, lane % 7 == 0] = 0.01
    gaps = rs.uniform(0.008, 0.012, (n_records, B))
    back = np.cumsum(gaps[::-1], axis=0)[::-1]           # distance from record i to the lead's newest
    d = lead[10][None, :] - back
    ang = rs.uniform(0, 2 * np.pi, B)
    direction = np.stack((np.cos(ang), np.sin(ang)), axis=-1)
    stretch = np.where(lane % 5 == 3, 8.0, 1.0)
    p = lead[0:2].T[None] - (stretch[None, :] * back)[..., None] * direction[None] + 0.002 * rs.standard_normal((n_records, B, 2))
    if periodic:
        p = p % 1.0
    return lead, d, p


@pytest.mark.parametrize("periodic", [False, True], ids=["solid", "periodic"])
@pytest.mark.parametrize("branch,n_records,phase", STEP_CASES, ids=[f"{b}-rec{r}-ph{p}" for b, r, p in STEP_CASES])
@pytest.mark.parametrize("B,n", SHAPES, ids=SHAPE_IDS)
def test_theta_sequence_step(riab, B, n, branch, n_records, phase, periodic):
    """ring [8][3][B], capacity = lookback = 8, with 0, 7, 8 and 9 records before the call (the wrap, and the first slot
    reused): the one slot n_records % 8 is written, with the lead's (distance, x, y) bit for bit, and every other slot
    keeps the bits it held — the records of the earlier steps, or the canary where there was none (`written=` on the
    first lap of the ring: the slot due and the slots already filled, no other).  pos_out [2][B] fully written; lead_state, future and count not a bit changed; diag counts the
    lanes < n_agents only (the padding lanes hold agents that raise and are dropped like the others).  Positions: NaN where
    the oracle's are, else within 1e-12 (tests/test_gpu_subagent.py test_sweep_interpolation_given_the_kernels_tables and
    the look-behind of test_sweep_against_the_oracles_own_rollouts); look-ahead with the table and counts the rollout
    kernel wrote, in the arena views it wrote them to.  NaN / 3e38 in every float input of the lanes >= n_agents change
    no bit of a lane < n_agents and no counter."""
    L = riab._lib
    ahead = branch == "ahead"
    lead, rec_d, rec_p = step_inputs(B, n_records, periodic, ahead)
    oenv = orc.EnvSpec(boundary_conditions="periodic" if periodic else "solid")
    env_obj = riab.Environment({"boundary_conditions": "periodic"} if periodic else {})
    env, _walls = env_obj.device_tables(torch.device("cuda"))
    t = 0.3 + phase * 0.1
    code = {"none": L.THETA_NONE, "behind": L.THETA_BEHIND, "ahead": L.THETA_AHEAD}[branch]
    slot = n_records % RING
    kept = np.arange(RING) != slot

    def run(canary, poison=None):
        arena = ga.GuardArena(canary)
        roll = Rollout(riab, B, n, canary, False) if ahead else None
        table = count = None
        if ahead:
            count = roll.arena.check(roll.count)
            if poison is not None:                       # (the padding lanes' table: their count stays what it was)
                roll.future[:, :, n:] = poison
            table = roll.future.cpu().numpy()            # (entries past count[b] hold the canary)
        lead_in = lead if poison is None else poisoned(lead, n, poison)
        lead_t = put(arena, lead_in)
        ring = arena.view((RING, 3, B), torch.float64, "cuda")
        for i in range(max(0, n_records - RING), n_records):
            rec = np.concatenate((rec_d[i][None], rec_p[i].T))
            ring[i % RING] = dev(rec if poison is None else poisoned(rec, n, poison))
        filled = np.zeros(RING, dtype=bool)
        filled[[i % RING for i in range(max(0, n_records - RING), n_records)]] = True
        held = ring.cpu().numpy()
        out = arena.view((2, B), torch.float64, "cuda")
        diag = put(arena, np.zeros(4, dtype=np.int32))
        phase_arg = (t % (1 / 10.0)) / (1 / 10.0)
        call(L, "riab_theta_sequence_step", env, L.ptr(lead_t), B, n, L.ptr(ring), RING, RING, n_records, code, phase_arg,
             D_HALF, 0.5, L.ptr(roll.future) if ahead else None, L.ptr(roll.count) if ahead else None, K_ROLL, L.ptr(out),
             L.ptr(diag), L.current_stream())
        pos = arena.check(out)
        if n_records < RING:          # the first lap: the slots no record has reached yet must still hold the canary
            now = arena.check(ring, written=np.broadcast_to((filled | ~kept)[:, None, None], (RING, 3, B)).copy())
        else:
            now = arena.check(ring, inplace=True)
        moved = np.argwhere(bits(now)[kept] != bits(held)[kept])
        assert len(moved) == 0, f"{len(moved)} elements of the slots other than {slot} changed, first at (kept slot, row, lane) {moved[0]}"
        np.testing.assert_array_equal(bits(now[slot]), bits(lead_in[[10, 0, 1]]))
        unchanged(arena, lead_t, lead_in)
        if ahead:                                        # the table and the counts: guards intact, not a bit changed
            roll.arena.check(roll.count, other=count)
            roll.arena.check(roll.future, inplace=True, other=table)
        return pos, arena.check(diag, inplace=True), table, count

    runs = [run(canary) for canary in ga.CANARIES]
    pos, diag, table, count = runs[0]
    np.testing.assert_array_equal(bits(runs[1][0]), bits(pos))
    np.testing.assert_array_equal(runs[1][1], diag)

    def oracle(lanes):
        o = sao.ThetaSequenceOracle(oenv, lanes, DT_LEAD, 0.08, v_sequence=V_SEQUENCE)
        o.lookback, o.K = RING, K_ROLL
        assert o.d_half == D_HALF and o.theta_frac == 0.5 and o.theta_freq == 10.0
        o.rec_d[:n_records], o.rec_p[:n_records], o.n_rec = rec_d[:, :lanes], rec_p[:, :lanes], n_records
        ld = lead_dict(lead[:, :lanes])
        return o, o.step(ld, t, future=(table[:, :, :lanes], count[:lanes]) if ahead else None)

    o, ref = oracle(B)
    assert {"none": True, "behind": 0.25 <= o.phase(t) < 0.5, "ahead": 0.5 <= o.phase(t) < 0.75}[branch]
    np.testing.assert_array_equal(np.isnan(pos.T), np.isnan(ref))
    if branch == "none":
        assert np.isnan(pos).all()
    else:
        err = np.nanmax(np.abs(pos.T - ref)) if np.isfinite(ref).any() else 0.0
        assert err <= 1e-12, err
    o_n, _ = oracle(n)
    assert diag.tolist() == [o_n.raises["behind"], o_n.raises["ahead"], 0, o_n.raises["far"]], (diag, o_n.raises)
    if branch == "behind" and n_records >= 7 and B > 4:      # every branch of the look-behind was met by a real lane
        fin = np.isfinite(ref[:n, 0])
        assert fin[0::2].all() and fin[1::2].any() and o_n.raises["far"] > 0
    for value in POISON:
        p_pos, p_diag, _t, _c = run("nan", poison=value)
        np.testing.assert_array_equal(bits(p_pos[:, :n]), bits(pos[:, :n]))
        np.testing.assert_array_equal(p_diag, diag)


# ---------------------------------------------------------------------------------------------------------------------
# riab_dumb_agent_step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("philox", [False, True], ids=["explicit", "philox"])
@pytest.mark.parametrize("kind", ["wall", "periodic"])
@pytest.mark.parametrize("B,n", SHAPES, ids=SHAPE_IDS)
def test_dumb_agent_step(riab, B, n, kind, philox):
    """3 consecutive steps in the walled box and the periodic box of tests/test_gpu_replay.py, on a lead that stays where
    the spring meets the room (that file's lead_path) and from displacements of the spring's own size, so that walls cut
    and the boundary conditions act within three steps.  displacement and velocity [2][B] in place; z_out and pos_out
    [2][B] fully written; lead_state and z_in not a bit changed.  After every step the three are the oracle's, stepped
    from the device's own previous state with the same normals, to 1e-12, and the counters are the oracle's over the lanes
    < n_agents (test_dumb_agent_one_step_parity)."""
    L = riab._lib
    rs = np.random.RandomState(31 * B + (kind == "wall"))
    env_obj = box(riab, kind)
    env, _walls = env_obj.device_tables(torch.device("cuda"))
    path = lead_path(kind, B, 3, rs)
    disp0, vel0 = 0.03 * rs.standard_normal((2, B)), 0.05 * rs.standard_normal((2, B))
    zs = rs.standard_normal((3, 2, B))
    o = rpo.DumbAgentOracle(oracle_box(kind), B, REPLAY_DT)
    theta, sigma = 1 / o.tau_v, np.sqrt((2 * o.sigma ** 2) / (o.tau_v * REPLAY_DT))
    seed, id0 = 0x1234567800000321, 4096
    runs = []
    for canary in ga.CANARIES:
        arena = ga.GuardArena(canary)
        disp, vel = put(arena, disp0), put(arena, vel0)
        diag = put(arena, np.zeros(4, dtype=np.int32))
        steps = []
        for t in range(3):
            lead = lead_rows(B, np.random.RandomState(t))
            lead[0:2] = path[t].T
            lead_t, z_in = put(arena, lead), put(arena, zs[t])
            z_out, out = (arena.view((2, B), torch.float64, "cuda") for _ in range(2))
            call(L, "riab_dumb_agent_step", env, L.ptr(lead_t), B, n, id0, L.ptr(disp), L.ptr(vel), REPLAY_DT, theta, sigma,
                 o.acceleration_scale, None if philox else L.ptr(z_in), L.ptr(z_out), seed, 5 + t, L.ptr(out), L.ptr(diag),
                 L.current_stream())
            unchanged(arena, lead_t, lead)
            unchanged(arena, z_in, zs[t])
            steps.append(dict(z=arena.check(z_out), pos=arena.check(out), disp=arena.check(disp, inplace=True),
                              vel=arena.check(vel, inplace=True)))
        runs.append((steps, arena.check(diag, inplace=True)))
    (steps, diag), (steps2, diag2) = runs
    np.testing.assert_array_equal(diag, diag2)
    o.displacement, o.displacement_velocity = disp0.T.copy(), vel0.T.copy()
    cuts = moved = 0
    for t in range(3):
        for key in ("z", "pos", "disp", "vel"):
            np.testing.assert_array_equal(bits(steps[t][key]), bits(steps2[t][key]), err_msg=f"step {t} {key}: canary-dependent")
        if philox:
            assert np.isfinite(steps[t]["z"]).all() and len(np.unique(steps[t]["z"])) == 2 * B
        else:
            np.testing.assert_array_equal(bits(steps[t]["z"]), bits(zs[t]))
        ref = o.step(path[t], steps[t]["z"])
        assert np.abs(steps[t]["pos"].T - ref).max() <= 1e-12
        assert np.abs(steps[t]["disp"].T - o.displacement).max() <= 1e-12
        assert np.abs(steps[t]["vel"].T - o.displacement_velocity).max() <= 1e-12
        cuts, moved = cuts + int(o.cut[:n].sum()), moved + int(o.outside[:n].sum())
        o.displacement, o.displacement_velocity = steps[t]["disp"].T.copy(), steps[t]["vel"].T.copy()
    assert diag.tolist() == [cuts, moved, 0, 0], (diag, cuts, moved)
    if B > 4 and not philox:
        assert (o.n_wall_cuts if kind == "wall" else o.n_boundary) >= 1


# ---------------------------------------------------------------------------------------------------------------------
# rate maps: riab_history_bin_index, riab_history_rate_map, riab_history_rate_map_finish
# ---------------------------------------------------------------------------------------------------------------------
GRIDS = {"1x1": (1, 1), "3x5": (3, 5), "64x64": (64, 64)}            # (nx, ny); 64 x 64 = RIAB_RATEMAP_MAX_BINS


def untouched(arena, view):
    """both guards intact and every element of the view still the canary"""
    arena.check(view, written=np.zeros(tuple(view.shape), dtype=bool))


def ratemap_inputs(T, n, B, n_real, grid):
    nx, ny = GRIDS[grid]
    rs = np.random.RandomState(1000 * B + 10 * n + T + nx)
    ex, ey = np.arange(nx + 1) / nx, np.arange(ny + 1) / ny
    x = rs.uniform(-0.1, 1.1, size=(T, B)).astype(np.float32)         # some samples fall outside
    y = rs.uniform(-0.1, 1.1, size=(T, B)).astype(np.float32)
    x[:, n_real:], y[:, n_real:] = 0.5, 0.5                           # the padding lanes stand inside the room
    traj = np.full((T, 8, B), 0.5, dtype=np.float32)
    traj[:, 0], traj[:, 1] = x, y
    rows = (rs.randint(0, 32, size=(T, n, B)) / 32.0).astype(np.float32)   # k / 32: every sum is exact in any order
    rows[:, :, n_real:] = 3.0e38
    return ex, ey, traj, rows


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("B,n_real", [(4, 4), (8, 5), (68, 68)], ids=["B4-r4", "B8-r5", "B68-r68"])
@pytest.mark.parametrize("n", [1, 5, 33])
@pytest.mark.parametrize("T", [1, 3])
def test_rate_maps(riab, T, n, B, n_real, grid):
    """bin_ids uint16 [T][B] fully written, the padding lanes RIAB_RATEMAP_DROPPED; counts int64 [ny][nx] and sums float64
    [n][n_bins] in place, pre-zeroed, a second call accumulating, their guards intact; the workspace exactly
    riab_history_rate_map_workspace doubles: its guards; with one double fewer the call returns RIAB_EINVAL and sums and
    workspace keep their canary everywhere; maps and zero_bins of the finishing call fully written; hist, edges and rows not
    a bit changed.  Ids by the searchsorted rule, counts, sums, maps and zero_bins bit for bit tests/ratemap_oracle.py's on
    exact samples (tests/test_gpu_ratemap.py test_edges and test_shapes_bit_for_bit; two calls: test_two_calls_accumulate_like_one).
    NaN / 3e38 in the positions and rates of the lanes >= n_real change no bit of an id of a lane < n_real, of counts or of
    sums."""
    L = riab._lib
    assert GRIDS["64x64"][0] * GRIDS["64x64"][1] == L.RATEMAP_MAX_BINS and L.RATEMAP_DROPPED == 0xFFFF
    nx, ny = GRIDS[grid]
    n_bins = nx * ny
    ex, ey, traj, rows = ratemap_inputs(T, n, B, n_real, grid)
    edges = np.concatenate((ex, ey))
    need = int(L.lib.riab_history_rate_map_workspace(T, n, B, n_bins))
    assert need >= n * n_bins
    stream = L.current_stream()

    def run(canary, traj, rows, finish=True):
        arena = ga.GuardArena(canary)
        hist_t, edges_t, rows_t = put(arena, traj), put(arena, edges), put(arena, rows)
        ids = arena.view((T, B), torch.uint16, "cuda")
        counts = put(arena, np.zeros((ny, nx), dtype=np.int64))
        sums = put(arena, np.zeros((n, n_bins)))
        ws = arena.view((need,), torch.float64, "cuda")
        out = {}
        for rep in (1, 2):
            call(L, "riab_history_bin_index", L.ptr(hist_t), T, B, n_real, ex.ctypes.data, nx, ey.ctypes.data, ny, L.ptr(edges_t),
                 L.ptr(ids), L.ptr(counts), stream)
            call(L, "riab_history_rate_map", L.ptr(rows_t), 0, T, n, B, L.ptr(ids), n_bins, L.ptr(sums), L.ptr(ws), need, stream)
            out[f"ids{rep}"] = arena.check(ids)
            out[f"counts{rep}"] = arena.check(counts, inplace=True)
            out[f"sums{rep}"] = arena.check(sums, inplace=True)
            arena.check(ws, inplace=True)
        if finish:
            maps, zero = arena.view((n, n_bins), torch.float64, "cuda"), arena.view((n_bins,), torch.uint8, "cuda")
            call(L, "riab_history_rate_map_finish", L.ptr(sums), L.ptr(counts), n, n_bins, 1, L.ptr(maps), L.ptr(zero), stream)
            out["maps"], out["zero"] = arena.check(maps), arena.check(zero)
            assert np.array_equal(bits(arena.check(sums, inplace=True)), bits(out["sums2"]))      # left as they are
            assert np.array_equal(arena.check(counts, inplace=True), out["counts2"])
        for v, a in ((hist_t, traj), (edges_t, edges), (rows_t, rows)):
            unchanged(arena, v, a)
        return out

    first = run("nan", traj, rows)
    second = run("finite", traj, rows)
    for k in first:
        np.testing.assert_array_equal(bits(first[k]), bits(second[k]), err_msg=f"{k}: canary-dependent")
    # ---- the oracle
    for t in range(T):
        kx = rmo.searchsorted_bins(traj[t, 0, :n_real], ex)
        ky = rmo.searchsorted_bins(traj[t, 1, :n_real], ey)
        want = np.where((kx >= 0) & (ky >= 0), (ny - 1 - ky) * nx + kx, 0xFFFF)
        np.testing.assert_array_equal(first["ids1"][t, :n_real].astype(np.int64), want)
        assert (first["ids1"][t, n_real:] == 0xFFFF).all()
    np.testing.assert_array_equal(first["ids1"], first["ids2"])
    osums, ozero, ocnt = rmo.rate_maps(traj, rows, n_real, ex, ey, False)
    omaps, _, _ = rmo.rate_maps(traj, rows, n_real, ex, ey, True)
    assert np.array_equal(first["counts1"], ocnt.astype(np.int64)) and np.array_equal(first["counts2"], 2 * ocnt.astype(np.int64))
    assert np.array_equal(first["sums1"].reshape(n, ny, nx), osums) and np.array_equal(first["sums2"].reshape(n, ny, nx), 2 * osums)
    assert np.array_equal(first["maps"].reshape(n, ny, nx), omaps)
    assert np.array_equal(first["zero"].reshape(ny, nx).astype(bool), ozero) and (first["zero"] <= 1).all()
    # ---- one double too few: refused before anything is launched
    for canary in ga.CANARIES:
        arena = ga.GuardArena(canary)
        rows_t, ids = put(arena, rows), put(arena, first["ids1"].view(np.int16))
        sums = arena.view((n, n_bins), torch.float64, "cuda")
        ws = arena.view((max(need - 1, 1),), torch.float64, "cuda")
        rc = L.lib.riab_history_rate_map(L.ptr(rows_t), 0, T, n, B, L.ptr(ids), n_bins, L.ptr(sums), L.ptr(ws), need - 1, stream)
        torch.cuda.synchronize()
        assert rc == L.EINVAL, rc
        untouched(arena, sums)
        untouched(arena, ws)
        unchanged(arena, rows_t, rows)
        unchanged(arena, ids, first["ids1"].view(np.int16))
    # ---- padding poison
    if n_real < B:
        for value in POISON:
            bad_traj, bad_rows = traj.copy(), poisoned(rows, n_real, value)
            bad_traj[:, 0:2, n_real:] = value
            got = run("nan", bad_traj, bad_rows, finish=False)
            for k in ("counts1", "counts2", "sums1", "sums2"):
                np.testing.assert_array_equal(bits(got[k]), bits(first[k]), err_msg=f"{k} with {value} in the padding lanes")
            np.testing.assert_array_equal(got["ids1"][:, :n_real], first["ids1"][:, :n_real])
            assert (got["ids1"][:, n_real:] == 0xFFFF).all()


# ---------------------------------------------------------------------------------------------------------------------
# the stand-alone geometry queries (csrc/riab_env.hip)
# ---------------------------------------------------------------------------------------------------------------------
ONE_WALL = [[[0.5, 0.1], [0.5, 0.6]]]
L_ROOM = [[0, 0], [1, 0], [1, 0.5], [0.5, 0.5], [0.5, 1], [0, 1]]
HOLE = [[0.2, 0.15], [0.4, 0.15], [0.4, 0.35], [0.2, 0.35]]


def _sixty_walls():
    rs = np.random.RandomState(60)
    a = rs.uniform(0.05, 0.95, (60, 2))
    ang = rs.uniform(0, np.pi, 60)
    return np.stack((a, a + 0.08 * np.stack((np.cos(ang), np.sin(ang)), axis=-1)), axis=1).tolist()


ROOMS = {"solid": ({}, {}), "periodic": ({"boundary_conditions": "periodic"}, {"boundary_conditions": "periodic"}),
         "one_wall": ({"walls": ONE_WALL}, {"walls": ONE_WALL}),                                           # 5 walls
         "sixty_walls": ({"walls": _sixty_walls()}, {"walls": _sixty_walls()}),                            # 64 = RIAB_MAX_WALLS
         "l_room_hole": ({"boundary": L_ROOM, "holes": [HOLE]}, {"boundary": L_ROOM, "holes": [HOLE]})}


def room_in_arena(riab, arena, name):
    """(the RiabEnv struct with its wall table copied into an arena view, that view, its content, the oracle's EnvSpec)"""
    L = riab._lib
    env_obj = riab.Environment(dict(ROOMS[name][0]))
    env, walls = env_obj.device_tables(torch.device("cuda"))
    mine = L.RiabEnv()
    C.memmove(C.byref(mine), C.byref(env), C.sizeof(mine))
    if walls is None or walls.numel() == 0:                   # (the periodic box: no wall, no table)
        return env, None, None, orc.EnvSpec(**ROOMS[name][1])
    table = walls.cpu().numpy()
    view = put(arena, table)
    mine.walls = view.data_ptr()
    return mine, view, table, orc.EnvSpec(**ROOMS[name][1])


PAIRS = [(1, 1), (3, 257), (65537, 3)]


@pytest.mark.parametrize("N1,N2", PAIRS, ids=[f"{a}x{b}" for a, b in PAIRS])
@pytest.mark.parametrize("room,geometry", [("one_wall", "euclidean"), ("one_wall", "line_of_sight"), ("one_wall", "geodesic"),
                                           ("periodic", "euclidean")])
def test_env_pairwise(riab, room, geometry, N1, N2):
    """dist, vec_x and vec_y [N1][N2] fully written; the four position rows and the wall table not a bit changed.  One
    interior wall, so that every geometry is allowed, and the periodic box for the wrapped vectors.  (65537, 3) is the only
    case in the suite whose rows outnumber the grid's 65535: the `i += gridDim.y` stride.  Against oracle.env_distances /
    env_vectors_between to tests/test_gpu_parity.py test_environment_queries_vs_reference's rtol 1e-14 (distances) and
    atol 1e-15 (vectors)."""
    L = riab._lib
    rs = np.random.RandomState(N1 + N2)
    p1, p2 = rs.uniform(0, 1, (N1, 2)), rs.uniform(0, 1, (N2, 2))
    got = {}
    for canary in ga.CANARIES:
        arena = ga.GuardArena(canary)
        env, w_t, w, oenv = room_in_arena(riab, arena, room)
        ins = [put(arena, a) for a in (p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1])]
        dist, vx, vy = (arena.view((N1, N2), torch.float64, "cuda") for _ in range(3))
        call(L, "riab_env_pairwise", env, L.ptr(ins[0]), L.ptr(ins[1]), N1, L.ptr(ins[2]), L.ptr(ins[3]), N2, L.GEOMETRIES[geometry],
             L.ptr(dist), L.ptr(vx), L.ptr(vy), L.current_stream())
        for k, v in (("dist", dist), ("vx", vx), ("vy", vy)):
            got[k] = arena.check(v, other=got.get(k))
        for v, a in zip(ins + [w_t], (p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1], w)):
            unchanged(arena, v, a)
    np.testing.assert_allclose(got["dist"], orc.env_distances(oenv, p1, p2, geometry), rtol=1e-14)
    vec = orc.env_vectors_between(oenv, p1, p2)
    np.testing.assert_allclose(got["vx"], vec[..., 0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(got["vy"], vec[..., 1], rtol=0, atol=1e-15)
    if geometry == "line_of_sight" and N1 * N2 > 100:
        assert (got["dist"] == 1000).any() and (got["dist"] < 1000).any()


@pytest.mark.parametrize("P", [1, 257])
@pytest.mark.parametrize("room", ["one_wall", "sixty_walls"])
def test_env_wall_queries(riab, room, P):
    """riab_env_vectors_from_walls: out [n_walls][2][P] float64 fully written; riab_env_check_wall_collisions: out
    [n_walls][P] uint8 fully written; at 5 walls and at 64 (RIAB_MAX_WALLS); positions and the wall table not a bit
    changed.  Vectors against oracle.shortest_vectors_from_walls to test_environment_queries_vs_reference's rtol 1e-12,
    atol 1e-15; the collision flags exactly (oracle.segment_intercepts, both parameters strictly inside (0, 1))."""
    L = riab._lib
    rs = np.random.RandomState(P + len(room))
    pos = rs.uniform(0, 1, (P, 2))
    end = pos + rs.uniform(-0.2, 0.2, (P, 2))
    got = {}
    for canary in ga.CANARIES:
        arena = ga.GuardArena(canary)
        env, w_t, w, oenv = room_in_arena(riab, arena, room)
        n_walls = int(env.n_walls)
        assert n_walls == len(oenv.walls) == {"one_wall": 5, "sixty_walls": L.MAX_WALLS}[room]
        ins = [put(arena, a) for a in (pos[:, 0], pos[:, 1], end[:, 0], end[:, 1])]
        vec = arena.view((n_walls, 2, P), torch.float64, "cuda")
        hit = arena.view((n_walls, P), torch.uint8, "cuda")
        call(L, "riab_env_vectors_from_walls", env, L.ptr(ins[0]), L.ptr(ins[1]), P, L.ptr(vec), L.current_stream())
        call(L, "riab_env_check_wall_collisions", env, L.ptr(ins[0]), L.ptr(ins[1]), L.ptr(ins[2]), L.ptr(ins[3]), P, L.ptr(hit),
             L.current_stream())
        got["vec"], got["hit"] = arena.check(vec, other=got.get("vec")), arena.check(hit, other=got.get("hit"))
        for v, a in zip(ins + [w_t], (pos[:, 0], pos[:, 1], end[:, 0], end[:, 1], w)):
            unchanged(arena, v, a)
    want = orc.shortest_vectors_from_walls(pos, oenv.walls)                       # (P, n_walls, 2)
    np.testing.assert_allclose(got["vec"].transpose(2, 0, 1), want, rtol=1e-12, atol=1e-15)
    l_a, l_b = orc.segment_intercepts(oenv.walls, np.stack((pos, end), axis=1))  # (n_walls, P)
    crossed = (l_a > 0) & (l_a < 1) & (l_b > 0) & (l_b < 1)
    assert (got["hit"] <= 1).all() and np.array_equal(got["hit"].astype(bool), crossed)
    if P > 1:
        assert crossed.any() and not crossed.all()


@pytest.mark.parametrize("P", [1, 257])
@pytest.mark.parametrize("room", ["solid", "periodic", "l_room_hole"])
def test_env_boundary_conditions(riab, room, P):
    """pos_x, pos_y [P] in place, inside_out uint8 [P] fully written, the wall table not a bit changed; apply = 1 and the
    check alone (apply = 0, which must not move a position).  Flags exactly oracle.env_is_inside / env_needs_resample (1
    inside, 2 left to the caller's sampler, 0 clamped or wrapped); positions: unchanged bit for bit unless the flag is 0,
    then oracle.env_apply_boundary_conditions to test_environment_queries_vs_reference's atol 1e-15."""
    L = riab._lib
    rs = np.random.RandomState(P + len(room))
    pos = rs.uniform(-0.3, 1.3, (P, 2)) if P > 1 else np.array([[1.2, -0.1]])
    for apply in (1, 0):
        got = {}
        for canary in ga.CANARIES:
            arena = ga.GuardArena(canary)
            env, w_t, w, oenv = room_in_arena(riab, arena, room)
            x, y = put(arena, pos[:, 0]), put(arena, pos[:, 1])
            flags = arena.view((P,), torch.uint8, "cuda")
            call(L, "riab_env_boundary_conditions", env, L.ptr(x), L.ptr(y), P, L.ptr(flags), apply, L.current_stream())
            got["flags"] = arena.check(flags, other=got.get("flags"))
            got["x"] = arena.check(x, inplace=True, other=got.get("x"))
            got["y"] = arena.check(y, inplace=True, other=got.get("y"))
            unchanged(arena, w_t, w)
        inside, resample = orc.env_is_inside(oenv, pos), orc.env_needs_resample(oenv, pos)
        np.testing.assert_array_equal(got["flags"], np.where(inside, 1, np.where(resample, 2, 0)))
        moved = (got["flags"] == 0) & bool(apply)
        new = np.stack((got["x"], got["y"]), axis=-1)
        np.testing.assert_array_equal(bits(new[~moved]), bits(pos[~moved]))
        if moved.any():
            np.testing.assert_allclose(new[moved], orc.env_apply_boundary_conditions(oenv, pos[moved]), rtol=0, atol=1e-15)
            assert orc.env_is_inside(oenv, new[moved]).all()
        if P > 1:
            seen = set(got["flags"].tolist())
            assert seen == ({1, 2} if room == "l_room_hole" else {0, 1}), seen


# ---------------------------------------------------------------------------------------------------------------------
# riab_replay_agent_step
# ---------------------------------------------------------------------------------------------------------------------
K_REPLAY, T_NOW, FREQ_DT, MEAN_SPEED, MEAN_DURATION = 8, 1.0, 5.0 * REPLAY_DT, 0.15, 0.1
OUTSIDE, STARTING, INSIDE, ENDING = range(4)
# how far the newer record of the j-th lane inside a replay lies below the query of the call (m; a sham step is 0.0005 ..
# 0.0012 m): beyond it (no step), a few steps, and more than K steps can cover
REPLAY_GAPS = [0.002, -0.0005, 0.015, 0.0004, 0.001, 0.003, 0.004, 0.005, 0.006, 0.0075]


def replay_inputs(B):
    """One call that holds lanes in four states, lane b in state b % 4: outside a replay (flag 0, u > freq_dt), starting one
    (flag 0, u <= freq_dt), inside one (flag 1, t < its end) and ending one (flag 1, t >= its end).  The lanes inside a
    replay are consistent — the newer record is the sham agent's own position and distance — and lie between "the newer
    record is already beyond the query" (no step) and "0.015 m short of it" (more than K = 8 sham steps cover: the lane
    runs out), by REPLAY_GAPS."""
    rs = np.random.RandomState(4000 + B)
    L = np.arange(B) % 4
    lead = lead_rows(B, rs)
    sham = lead_rows(B, rs, speed=rs.uniform(0.05, 0.12, B))
    sham[0:2] = rs.uniform(0.6, 0.9, (2, B))                         # (clear of the wall at x = 0.5, y < 0.5)
    flag = np.isin(L, (INSIDE, ENDING)).astype(np.int32)
    rp = np.zeros((10, B))
    rp[0] = rs.uniform(0.25, 0.3, B)                                 # RIAB_RP_SPEED
    rp[1] = T_NOW - rs.uniform(0.07, 0.1, B)                         # RIAB_RP_T_START: the query is 0.0175 m at least
    rp[2] = np.where(L == ENDING, T_NOW - rs.uniform(0.0, 0.01, B), T_NOW + 0.05)        # RIAB_RP_T_END (one lane: t == end)
    rp[2, 3] = T_NOW
    query = rp[0] * (T_NOW - rp[1])
    hi_d = query - np.array(REPLAY_GAPS)[(np.arange(B) // 4) % len(REPLAY_GAPS)]
    rp[3] = sham[10] - hi_d                                          # RIAB_RP_D_START
    rp[7], rp[8], rp[9] = hi_d, sham[0], sham[1]                     # RIAB_RP_HI: the sham agent's newest step
    rp[4], rp[5], rp[6] = hi_d - 0.0008, sham[0] - 0.0005, sham[1] + 0.0006             # RIAB_RP_LO
    rp[:, L == OUTSIDE] = rs.uniform(0, 1, (10, int((L == OUTSIDE).sum())))              # what an ended replay left behind
    draws = np.stack((np.where(L == STARTING, rs.uniform(0, FREQ_DT, B), rs.uniform(FREQ_DT + 1e-3, 1, B)),
                      rs.rayleigh(MEAN_SPEED, B), rs.rayleigh(MEAN_DURATION, B), rs.uniform(0.55, 0.95, B), rs.uniform(0.05, 0.95, B),
                      rs.uniform(0, 2 * np.pi, B)))
    draws[2, 1] = 0.01                                               # a duration below its floor of mean / 2
    z = rs.standard_normal((K_REPLAY, 2, B))
    return L, lead, sham, flag, rp, draws, z


@pytest.mark.parametrize("B,n", SHAPES, ids=SHAPE_IDS)
def test_replay_agent_step(riab, B, n):
    """flag, steps_taken [B] and pos_out [2][B] fully written; replay_state [10][B] and sham_state [12][B] in place;
    draws_out [6][B] fully written and NaN exactly where no draw was taken; z_out [K][2][B] in the rows below its wave's
    last step and in no other; lead_state, draws_in and z_in not a bit changed.  The interior as tests/test_gpu_replay.py
    has it: records and sham state bit for bit riab_agent_step(T = 1) from the same start, idle lanes' state kept
    (replay_run, G3); pos_out the interpolation of the records to 1e-12 (test_replay_is_the_motion_kernel); flags the
    oracle's and positions within 4 x the deviation of riab_agent_step from oracle.agent_step over the same steps, floor
    1e-12, the oracle fed what the kernel used, no step count it would have chosen differently
    (test_replay_against_the_oracle); counters over the lanes < n_agents."""
    L = riab._lib
    state_of, lead, sham0, flag0, rp0, draws, z = replay_inputs(B)
    np.random.seed(6)
    env_obj = box(riab, "wall")
    sham_agent = riab.Agent(env_obj, {"n_agents": n, "dt": REPLAY_DT})
    assert sham_agent._Bp == B
    env, _walls = env_obj.device_tables(sham_agent._device)
    m = sham_agent._motion(REPLAY_DT, False, 1, {})
    speed_mean, id0, seed = float(sham_agent.speed_mean), 4096, int(sham_agent.rng_seed)
    got = {}
    for canary in ga.CANARIES:
        a = ga.GuardArena(canary)
        lead_t, draws_t, z_t = put(a, lead), put(a, draws), put(a, z)
        sham_t, flag_t, rp_t = put(a, sham0), put(a, flag0), put(a, rp0)
        diag = put(a, np.zeros(4, dtype=np.int32))
        draws_out = a.view((6, B), torch.float64, "cuda")
        z_out = a.view((K_REPLAY, 2, B), torch.float64, "cuda")
        out = a.view((2, B), torch.float64, "cuda")
        steps = a.view((B,), torch.int32, "cuda")
        call(L, "riab_replay_agent_step", env, m, L.ptr(lead_t), L.ptr(sham_t), B, n, id0, L.ptr(flag_t), L.ptr(rp_t), T_NOW,
             FREQ_DT, MEAN_SPEED, MEAN_DURATION, speed_mean, L.ptr(draws_t), L.ptr(draws_out), seed, 11, L.ptr(z_t), L.ptr(z_out),
             seed, 11 * K_REPLAY, K_REPLAY, L.ptr(out), L.ptr(steps), None, L.ptr(diag), L.current_stream())
        n_steps = a.check(steps, other=got.get("steps"))
        last = np.array([n_steps[w * 64:(w + 1) * 64].max() for w in range((B + 63) // 64)])
        m_z = np.broadcast_to((np.arange(K_REPLAY)[:, None] < last[np.arange(B) // 64][None, :])[:, None, :], (K_REPLAY, 2, B)).copy()
        got = dict(steps=n_steps, m_z=m_z, z_out=a.check(z_out, written=m_z, other=got.get("z_out")),
                   flag=a.check(flag_t, inplace=True, other=got.get("flag")), pos=a.check(out, other=got.get("pos")),
                   draws=a.check(draws_out, other=got.get("draws")), rp=a.check(rp_t, inplace=True, other=got.get("rp")),
                   sham=a.check(sham_t, inplace=True, other=got.get("sham")), diag=a.check(diag, inplace=True, other=got.get("diag")))
        for v, x in ((lead_t, lead), (draws_t, draws), (z_t, z)):
            unchanged(a, v, x)
    n_steps, pos, used, rp, sham, flag = got["steps"], got["pos"].T, got["draws"], got["rp"], got["sham"], got["flag"]
    is_ = {k: state_of == k for k in range(4)}
    # ---- which lanes did what
    np.testing.assert_array_equal(flag, (is_[STARTING] | is_[INSIDE]).astype(np.int32))
    assert (n_steps[~is_[INSIDE]] == 0).all() and 0 <= n_steps.min() and n_steps.max() <= K_REPLAY
    if B > 4:
        assert {0, K_REPLAY} <= set(n_steps[is_[INSIDE]].tolist()) and len(set(n_steps[:64].tolist())) >= 5
    # ---- draws_out: NaN exactly where no draw was taken
    drew_u, drew_rest = is_[OUTSIDE] | is_[STARTING], is_[STARTING]
    np.testing.assert_array_equal(np.isnan(used[0]), ~drew_u)
    np.testing.assert_array_equal(np.isnan(used[1:]), np.broadcast_to(~drew_rest, (5, B)))
    np.testing.assert_array_equal(bits(used[0][drew_u]), bits(draws[0][drew_u]))
    np.testing.assert_array_equal(bits(used[1:][:, drew_rest]), bits(draws[1:][:, drew_rest]))
    np.testing.assert_array_equal(bits(got["z_out"][got["m_z"]]), bits(z[got["m_z"]]))
    # ---- state: kept, started, or the motion kernel's
    keep = is_[OUTSIDE] | is_[ENDING]
    np.testing.assert_array_equal(bits(rp[:, keep]), bits(rp0[:, keep]))
    np.testing.assert_array_equal(bits(sham[:, keep]), bits(sham0[:, keep]))
    np.testing.assert_array_equal(bits(pos[keep]), bits(lead[0:2].T[keep]))
    s = is_[STARTING]
    want_rp = np.stack((draws[1], np.full(B, T_NOW), T_NOW + np.maximum(draws[2], MEAN_DURATION / 2), sham0[10], np.zeros(B), draws[3],
                        draws[4], np.zeros(B), draws[3], draws[4]))
    np.testing.assert_array_equal(bits(rp[:, s]), bits(want_rp[:, s]))
    np.testing.assert_array_equal(bits(pos[s]), bits(draws[3:5].T[s]))
    other_rows = [r for r in range(12) if r not in (L.S_POS_X, L.S_POS_Y, L.S_VEL_X, L.S_VEL_Y, L.S_ROT_VEL)]
    np.testing.assert_array_equal(bits(sham[other_rows][:, s]), bits(sham0[other_rows][:, s]))
    np.testing.assert_array_equal(bits(sham[[L.S_POS_X, L.S_POS_Y]][:, s]), bits(draws[3:5][:, s]))
    assert (sham[L.S_ROT_VEL][s] == 0).all() and np.isfinite(sham[L.S_VEL_X:L.S_VEL_Y + 1][:, s]).all()
    ref = agent_steps(L, env, m, B, id0, dev(sham0), int(n_steps.max()), dev(z), seed, 0)
    interp_err = 0.0
    for b in np.nonzero(is_[INSIDE])[0]:
        k, d0 = int(n_steps[b]), rp[L.RP_D_START, b]
        assert d0 == rp0[L.RP_D_START, b] and (rp[0:3, b] == rp0[0:3, b]).all()
        if k:
            hi = (ref[k, L.S_DIST, b] - d0, ref[k, L.S_POS_X, b], ref[k, L.S_POS_Y, b])
            lo = (ref[k - 1, L.S_DIST, b] - d0, ref[k - 1, L.S_POS_X, b], ref[k - 1, L.S_POS_Y, b]) if k > 1 else tuple(rp0[7:10, b])
            np.testing.assert_array_equal(rp[7:10, b], hi, err_msg=f"lane {b}: newer record")
            np.testing.assert_array_equal(rp[4:7, b], lo, err_msg=f"lane {b}: older record")
        else:
            np.testing.assert_array_equal(bits(rp[:, b]), bits(rp0[:, b]))
        np.testing.assert_array_equal(bits(sham[:, b]), bits(ref[k, :, b]), err_msg=f"lane {b}: sham state")
        q = rp[0, b] * (T_NOW - rp[1, b])
        lo, hi = rp[4:7, b], rp[7:10, b]
        if hi[0] >= q:
            assert lo[0] < q or k == 0
            want = (hi[1:] - lo[1:]) / (hi[0] - lo[0]) * (q - lo[0]) + lo[1:]
            interp_err = max(interp_err, np.abs(pos[b] - want).max())
        else:
            assert k == K_REPLAY
            np.testing.assert_array_equal(pos[b], hi[1:])           # out of steps: the newest record
    assert interp_err <= 1e-12, interp_err
    saturated = is_[INSIDE] & ~(rp[7] >= rp[0] * (T_NOW - rp[1]))
    assert saturated.any() or B == 4
    assert got["diag"].tolist() == [int(s[:n].sum()), int(is_[ENDING][:n].sum()), int(saturated[:n].sum()), 0], got["diag"]
    # ---- the oracle, fed what the kernel used
    o = rpo.ReplayAgentOracle(oracle_box("wall"), B, REPLAY_DT, "lazy", None, 5.0, MEAN_DURATION, MEAN_SPEED, steps_max=K_REPLAY,
                              sham_state=sham_state_dict(sham0))
    assert o.speed_mean == speed_mean and o.replay_freq * o.dt == FREQ_DT
    o.flag, o.speed, o.t_start, o.t_end, o.d_start = flag0.astype(bool), rp0[0].copy(), rp0[1].copy(), rp0[2].copy(), rp0[3].copy()
    o.lo_d, o.lo_p, o.hi_d, o.hi_p = rp0[4].copy(), rp0[5:7].T.copy(), rp0[7].copy(), rp0[8:10].T.copy()
    fed = dict(u=np.where(np.isnan(used[0]), 2.0, used[0]), speed=used[1], duration=used[2], pos=used[3:5], direction=used[5])
    want = o.step(lead[0:2].T, T_NOW, draws=fed, z=np.where(got["m_z"], got["z_out"], 0.0), n_steps=n_steps)
    np.testing.assert_array_equal(flag.astype(bool), o.flag)
    stepped = n_steps > 0
    dev_motion = max(np.abs(rp[7][stepped] - o.hi_d[stepped]).max(), np.abs(rp[8:10].T[stepped] - o.hi_p[stepped]).max())
    bound = max(4 * dev_motion, FLOOR)
    err = np.abs(pos - want).max()
    print(f"[replay B={B}] steps {np.bincount(n_steps[is_[INSIDE]], minlength=K_REPLAY + 1).tolist()}, saturated {int(saturated.sum())}; "
          f"interpolation {interp_err:.3g} (bound 1e-12); riab_agent_step against oracle.agent_step {dev_motion:.3g}; positions "
          f"against the oracle {err:.3g} (bound {bound:.3g})")
    assert err <= bound and o.steps_disagree == 0
    assert (o.n_started, o.n_ended, o.saturations) == (int(s.sum()), int(is_[ENDING].sum()), int(saturated.sum()))


# ---------------------------------------------------------------------------------------------------------------------
# ring-buffer rates: simulate() of a population that does not save its history
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [3, 300])
def test_ring_buffer_rates(riab, monkeypatch, T):
    """256 agents x 9 PlaceCells with save_history=False (tests/test_gpu_guard_bands.py test_streamed_and_planned_forms'
    sizes): the rates stream through a ring of at most 256 rows that `Neurons._reserve_rows_at` / `_reserve_rows` allocate
    at its exact size, so nothing behind it is the package's to check.  Both are patched here, test-side only, to hand back
    an arena view of the shape they would have allocated.  T = 3: a ring of 3 rows; T = 300: longer than the ring, the
    second piece starts again at the ring's first row.  Both guards intact, every row of the ring written, and
    `firingrate_tensor` after the run is the oracle on the last history position (assert_rates, scale 30: the bound of
    test_streamed_and_planned_forms); `Agent.last_rate_stage_form()` says which form ran."""
    from ratinabox_amd.Neurons import Neurons
    from tests.test_gpu_parity import assert_rates
    B = 256
    first = None
    for canary in ga.CANARIES:
        arena, handed = ga.GuardArena(canary), []
        plain_at, plain = Neurons._reserve_rows_at, Neurons._reserve_rows

        def reserve_rows_at(self, n_steps, ring, _plain=plain_at, _arena=arena, _handed=handed):
            at = _plain(self, n_steps, ring)
            if at[4] is None:
                return at
            _handed.append(_arena.view(tuple(at[0].shape), at[0].dtype, "cuda"))
            return (_handed[-1],) + tuple(at[1:])

        def reserve_rows(self, n_steps, ring, _plain=plain, _arena=arena, _handed=handed):
            out = _plain(self, n_steps, ring)
            if out["ring"] is not None:
                _handed.append(_arena.view(tuple(out["fr"].shape), out["fr"].dtype, "cuda"))
                out["fr"] = _handed[-1]
            return out

        with monkeypatch.context() as mp:
            mp.setattr(Neurons, "_reserve_rows_at", reserve_rows_at)
            mp.setattr(Neurons, "_reserve_rows", reserve_rows)
            np.random.seed(11)
            env = riab.Environment({})
            Ag = riab.Agent(env, {"n_agents": B, "dt": 0.01, "seed": 0x1234567800000321, "agent_id0": 4096})
            np.random.seed(12)
            N = riab.PlaceCells(Ag, {"n": 9, "wall_geometry": "euclidean", "save_history": False, "max_fr": 30.0})
            Ag.simulate(T)
            torch.cuda.synchronize()
        form = Ag.last_rate_stage_form()
        assert form == "one-kernel", form
        assert Ag.diagnostics["pipeline_timeouts"] == 0
        assert len(handed) == 1 and tuple(handed[0].shape) == (min(T, 256), 9, B), [tuple(v.shape) for v in handed]
        ring = arena.check(handed[0])
        rates = N.firingrate_tensor.cpu().numpy()
        last = (T - 1) % 256 if T > 256 else T - 1                    # (every piece starts at the ring's first row)
        np.testing.assert_array_equal(bits(rates), bits(ring[last]))
        pos = np.asarray(Ag.history["pos"])[-1].astype(np.float32).astype(np.float64)      # (the rate kernels read fp32 rows)
        assert pos.shape == (B, 2) and len(np.asarray(Ag.history["pos"])) == T
        ref = orc.place_cells(orc.EnvSpec(), pos, N.place_cell_centres, N.place_cell_widths, wall_geometry="euclidean", max_fr=30.0)
        assert_rates(rates, ref, scale=30.0)
        if first is not None:
            np.testing.assert_array_equal(bits(rates), bits(first))
        first = rates


# ---------------------------------------------------------------------------------------------------------------------
# the task kernels: riab_task_reset / _step / _goal_vector and riab_task_world_reset / _step / _goal_vector
# ---------------------------------------------------------------------------------------------------------------------
TASK_GOALS = [[0.2, 0.25], [0.8, 0.7], [0.5, 0.12], [0.15, 0.85], [0.5, 0.5], [0.53, 0.5], [0.5, 0.54]]
TASK_WALLS = [[[0.5, 0.25], [0.5, 0.4]]]          # (the goals and the wall of tests/test_gpu_task_world.py)
TASK_SEED, TASK_ID0, TASK_DT, TASK_DELAY, EP_CAP = 11, 1000, 0.01, 0.005, 64


def task_setup(riab, arena, n_agents, goalorder, n_sel, shared):
    """The RiabEnv and RiabTask structs of a SpatialGoalEnvironment, their wall table and goal pool copied into arena
    views; the goal table for the oracle.  The class is used for the structs only: every launch below is a raw export on
    buffers of the test's own."""
    from ratinabox_amd.contribs.TaskEnvironment import SpatialGoalEnvironment
    L = riab._lib
    np.random.seed(2)
    kw = dict(lanes="agents") if shared else {}
    env = SpatialGoalEnvironment(params={"walls": TASK_WALLS}, possible_goal_positions=TASK_GOALS,
                                 goalcachekws=dict(reset_n_goals=n_sel, goalorder=goalorder), goalkws={"goal_radius": 0.06},
                                 episode_terminate_delay=TASK_DELAY, seed=TASK_SEED, **kw)
    Ag = riab.Agent(env, {"dt": TASK_DT, "n_agents": n_agents, "seed": 4, "agent_id0": TASK_ID0})
    env.add_agents(Ag)
    env_s, walls = env.device_tables(torch.device("cuda"))
    task_s = env._task_struct()
    mine_env, mine_task = L.RiabEnv(), L.RiabTask()
    C.memmove(C.byref(mine_env), C.byref(env_s), C.sizeof(mine_env))
    C.memmove(C.byref(mine_task), C.byref(task_s), C.sizeof(mine_task))
    w, pool = walls.cpu().numpy(), env._pool_dev.cpu().numpy()
    table = pool.copy()                   # rows (x, y, radius, the goal's Reward.row()): what the oracle takes
    np.testing.assert_array_equal(table[:, 0:2], TASK_GOALS)
    w_t, pool_t = put(arena, w), put(arena, pool)
    mine_env.walls, mine_task.goals = w_t.data_ptr(), pool_t.data_ptr()
    assert int(mine_task.n_pool) == len(TASK_GOALS)
    return mine_env, mine_task, [(w_t, w), (pool_t, pool)], table, (env, Ag)


def task_paths(B, Bp, lists, shared):
    """positions [3][2][Bp] after each of three steps.  Lanes: b % 4 == 0 stands in the first goal of its list at step 1
    and in the second at step 2 (its list is empty then, the termination delay runs out at step 3); 1: in its first goal
    from step 2 on; 2: nowhere near a goal; 3: at (0.512, 0.521), inside three goals at once.  One world: agents 0 and 1 in
    the first goal of the shared list at step 1 (the first in agent order gets it), the LAST agent in the second at step 2."""
    rs = np.random.RandomState(B)
    G = np.array(TASK_GOALS)
    pos = np.empty((3, 2, Bp))
    for k in range(3):
        p = np.tile([0.92, 0.3], (Bp, 1)) + rs.uniform(-0.02, 0.02, (Bp, 2))
        for b in range(B):
            first, second = (G[lists[b][0]], G[lists[b][1]])
            if shared:
                if b in (0, 1) and k == 0:
                    p[b] = first + [0.01 * b, 0.0]
                if b == B - 1 and k == 1:
                    p[b] = second + [0.0, 0.01]
            elif b % 4 == 0:
                p[b] = (first if k == 0 else second) + rs.uniform(-0.01, 0.01, 2)
            elif b % 4 == 1 and k >= 1:
                p[b] = first + rs.uniform(-0.01, 0.01, 2)
            elif b % 4 == 3:
                p[b] = [0.512, 0.521]
        pos[k] = p.T
    return pos


def goal_vector_reference(pos, goal_list, table, sequential):
    """get_goal_vector for one lane (tests/test_gpu_task_world.py test_task_world_many_agents_vs_oracle): the head of the
    list, or the nearest pending goal; None where the list holds the termination-delay goal (not compared there)"""
    if orc.GOAL_TIME_ELAPSED in goal_list:
        return None
    if not goal_list:
        return np.zeros(2)
    pend = np.array([table[e, 0:2] for e in goal_list])
    return pend[0] - pos if sequential else pend[np.argmin(np.linalg.norm(pend - pos, axis=1))] - pos


@pytest.mark.parametrize("goalorder", ["nonsequential", "sequential"])
@pytest.mark.parametrize("Bp,B", SHAPES, ids=[f"B{b}-n{n}" for b, n in SHAPES])
def test_task_lane_kernels(riab, Bp, B, goalorder):
    """riab_task_reset, three times riab_task_goal_vector + riab_task_step, then a masked riab_task_reset of the lanes that
    are terminal.  The task's arrays hold B = n_agents lanes, the position rows are the agent's, padded to Bp.  State
    [RIAB_TS_ROWS][B], the episode log and its counter and diag in place; reward, terminal and both goal-vector rows fully
    written; positions, mask, goal pool and wall table not a bit changed.  Goal lists exactly oracle.task_reset_draws
    (tests/test_gpu_task.py test_task_production_reset_matches_host_philox, masked lanes untouched); reward totals and
    terminal flags of EVERY lane bit for bit oracle.TaskLane's (test_agents_reach_their_goals_closed_loop: `total == r[b]
    and terminal == tm[b]`); goal vectors to test_task_world_many_agents_vs_oracle's rtol 1e-12, atol 1e-15.  NaN / 3e38 in
    the position entries b >= B change no bit of any of it."""
    L = riab._lib
    n_sel, n_pool, sequential = 2, len(TASK_GOALS), goalorder == "sequential"
    lists = [orc.task_reset_draws(TASK_SEED, 1, TASK_ID0 + b, n_pool, n_sel) for b in range(B)]
    paths = task_paths(B, Bp, lists, False)
    ts0 = np.zeros((L.TS_ROWS, B))
    ts0[L.TS_R_MAX], ts0[L.TS_R_MIN] = -np.inf, np.inf
    stream = L.current_stream()

    def run(canary, poison=None):
        a = ga.GuardArena(canary)
        env_s, task_s, tables, table, keep = task_setup(riab, a, B, goalorder, n_sel, False)
        ts = put(a, ts0)
        ep_log, ep_count, diag = put(a, np.zeros((EP_CAP, 5))), put(a, np.zeros(1, dtype=np.int32)), put(a, np.zeros(4, dtype=np.int32))
        out = dict(table=table)
        start = paths[0] if poison is None else poisoned(paths[0], B, poison)
        pos = put(a, start)
        call(L, "riab_task_reset", env_s, task_s, L.ptr(ts), None, B, TASK_ID0, 0.0, n_sel, 0, TASK_SEED, 1, 0, None, None,
             L.ptr(pos[0]), L.ptr(pos[1]), None, None, L.ptr(ep_log), EP_CAP, L.ptr(ep_count), L.ptr(diag), stream)
        out["reset"] = a.check(ts, inplace=True)
        unchanged(a, pos, start)
        t = 0.0
        for k in range(3):
            t = t + TASK_DT
            p = paths[k] if poison is None else poisoned(paths[k], B, poison)
            pos = put(a, p)
            gv, reward, terminal = a.view((2, B), torch.float64, "cuda"), a.view((B,), torch.float64, "cuda"), a.view((B,), torch.uint8, "cuda")
            call(L, "riab_task_goal_vector", env_s, task_s, L.ptr(ts), L.ptr(pos[0]), L.ptr(pos[1]), B, 0.0, L.ptr(gv[0]), L.ptr(gv[1]), stream)
            out[f"gv{k}"], out[f"ts_gv{k}"] = a.check(gv), a.check(ts, inplace=True)
            call(L, "riab_task_step", env_s, task_s, L.ptr(ts), L.ptr(pos[0]), L.ptr(pos[1]), B, t, L.ptr(reward), L.ptr(terminal),
                 L.ptr(diag), stream)
            out[f"reward{k}"], out[f"terminal{k}"], out[f"ts{k}"] = a.check(reward), a.check(terminal), a.check(ts, inplace=True)
            unchanged(a, pos, p)
        mask = out["terminal2"].copy()
        mask_t = put(a, mask)
        call(L, "riab_task_reset", env_s, task_s, L.ptr(ts), L.ptr(mask_t), B, TASK_ID0, t, n_sel, 0, TASK_SEED, 2, 0, None, None,
             L.ptr(pos[0]), L.ptr(pos[1]), None, None, L.ptr(ep_log), EP_CAP, L.ptr(ep_count), L.ptr(diag), stream)
        out["ts_end"], log = a.check(ts, inplace=True), a.check(ep_log, inplace=True)
        out["ep_count"], out["diag"] = a.check(ep_count, inplace=True), a.check(diag, inplace=True)
        n_log = int(out["ep_count"][0])
        log[:n_log] = log[:n_log][np.argsort(log[:n_log, 0])]      # (appended through an atomic counter: in lane order here)
        out["ep_log"] = log
        unchanged(a, mask_t, mask)
        unchanged(a, pos, p)
        for v, x in tables:
            unchanged(a, v, x)
        return out

    first, second = run("nan"), run("finite")
    for key in first:
        np.testing.assert_array_equal(bits(first[key]), bits(second[key]), err_msg=f"{key}: canary-dependent")
    table = first["table"]
    # ---- the first reset: every lane's list
    ts = first["reset"]
    assert (ts[L.TS_N_GOALS] == n_sel).all() and (ts[L.TS_EPISODE] == 1).all()
    np.testing.assert_array_equal(ts[L.TS_GOAL_LIST:L.TS_GOAL_LIST + n_sel].T.astype(int), np.array(lists))
    # ---- three steps, every lane against its TaskLane
    oenv = orc.EnvSpec(walls=TASK_WALLS)
    lanes = [orc.TaskLane(oenv, table, goalorder, TASK_DELAY) for _ in range(B)]
    for b in range(B):
        lanes[b].reset(0.0, lists[b])
    t = 0.0
    for k in range(3):
        t = t + TASK_DT
        np.testing.assert_array_equal(bits(first[f"ts_gv{k}"]), bits(first["reset"] if k == 0 else first[f"ts{k - 1}"]))  # reads only
        for b in range(B):
            want = goal_vector_reference(paths[k][:, b], lanes[b].goal_list, table, sequential)
            if want is not None:
                np.testing.assert_allclose(first[f"gv{k}"][:, b], want, rtol=1e-12, atol=1e-15, err_msg=f"step {k} lane {b}")
            total, terminal = lanes[b].step(paths[k][:, b], t)
            assert total == first[f"reward{k}"][b] and terminal == first[f"terminal{k}"][b], (k, b)
        assert (first[f"terminal{k}"] <= 1).all()
        np.testing.assert_array_equal(first[f"ts{k}"][L.TS_N_REWARDS], [len(x.rewards) for x in lanes])
    mask = first["terminal2"].astype(bool)
    if B > 3:
        assert mask.any() and not mask.all() and max(first[f"reward{k}"].max() for k in range(3)) > 0
    # ---- the masked reset
    end, before = first["ts_end"], first["ts2"]
    np.testing.assert_array_equal(bits(end[:, ~mask]), bits(before[:, ~mask]))
    for b in np.nonzero(mask)[0]:
        assert end[L.TS_GOAL_LIST:L.TS_GOAL_LIST + n_sel, b].astype(int).tolist() == orc.task_reset_draws(TASK_SEED, 2, TASK_ID0 + b, n_pool, n_sel)
        assert end[L.TS_N_GOALS, b] == n_sel and end[L.TS_EPISODE, b] == 2
    assert int(first["ep_count"][0]) == int(mask.sum())
    assert first["diag"].tolist() == [0, sum(x.late_completions for x in lanes), 0, B + int(mask.sum())], first["diag"]
    log = first["ep_log"][:int(mask.sum())]
    assert log[:, 0].astype(int).tolist() == (TASK_ID0 + np.nonzero(mask)[0]).tolist()
    np.testing.assert_array_equal(log[:, 1:], np.tile([1.0, 0.0, t, t], (len(log), 1)))
    # ---- padding poison: the position entries behind the task's B lanes
    if Bp > B:
        for value in POISON:
            got = run("nan", poison=value)
            for key in first:
                np.testing.assert_array_equal(bits(got[key]), bits(first[key]), err_msg=f"{key} with {value} behind lane B")


WORLD_SHAPES = SHAPES + [(260, 260)]       # 260: the first multiple of 4 past one WORLD_BLOCK (256, csrc/riab_task_world.hip)


@pytest.mark.parametrize("goalorder", ["nonsequential", "sequential"])
@pytest.mark.parametrize("Bp,B", WORLD_SHAPES, ids=[f"B{b}-n{n}" for b, n in WORLD_SHAPES])
def test_task_world_kernels(riab, Bp, B, goalorder):
    """The agents of ONE world: riab_task_world_reset, three times riab_task_world_goal_vector + riab_task_world_step, then
    a second reset that also writes the goal vectors.  Per-agent state [RIAB_TS_ROWS][B], the shared `world`
    [RIAB_TW_ROWS], episode log, counter and diag in place; reward and the goal-vector rows fully written; the terminal
    column in place from zeros (by its contract it is rewritten only when the world's flag changes); the met / candidate
    scratch: guards only; the ticket pair zero again after every launch; positions, pool and walls not a bit changed.
    B = 260 puts the last agent, who takes a goal, into a second workgroup.  Against oracle.TaskWorld as
    tests/test_gpu_task_world.py test_task_world_many_agents_vs_oracle asserts it: every agent's total bit for bit, the
    flag, the shared list, the reward counts, the goal vectors (rtol 1e-12, atol 1e-15), the lists of both resets exactly
    oracle.task_reset_draws.  NaN / 3e38 in the position entries b >= B change no bit."""
    L = riab._lib
    n_sel, n_pool, sequential = 2, len(TASK_GOALS), goalorder == "sequential"
    sel = orc.task_reset_draws(TASK_SEED, 1, 0xFFFFFFFF, n_pool, n_sel)
    paths = task_paths(B, Bp, [sel] * B, True)
    ts0 = np.zeros((L.TS_ROWS, B))
    ts0[L.TS_R_MAX], ts0[L.TS_R_MIN] = -np.inf, np.inf
    stream = L.current_stream()

    def run(canary, poison=None):
        a = ga.GuardArena(canary)
        env_s, task_s, tables, table, keep = task_setup(riab, a, B, goalorder, n_sel, True)
        ts, world = put(a, ts0), put(a, np.zeros(L.TW_ROWS))
        ep_log, ep_count, diag = put(a, np.zeros((EP_CAP, 5))), put(a, np.zeros(1, dtype=np.int32)), put(a, np.zeros(4, dtype=np.int32))
        terminal, ctl = put(a, np.zeros(B, dtype=np.uint8)), put(a, np.zeros(2, dtype=np.int32))
        met, cand = a.view((B,), torch.int64, "cuda"), a.view((B,), torch.int32, "cuda")
        out = dict(table=table)
        start = paths[0] if poison is None else poisoned(paths[0], B, poison)
        pos = put(a, start)
        call(L, "riab_task_world_reset", env_s, task_s, L.ptr(ts), L.ptr(world), B, TASK_ID0, 0.0, n_sel, 0, TASK_SEED, 1, 0, None,
             None, L.ptr(pos[0]), L.ptr(pos[1]), None, None, L.ptr(ep_log), EP_CAP, L.ptr(ep_count), 0, 0.0, None, None,
             L.ptr(diag), stream)
        out["world_reset"], out["ts_reset"] = a.check(world, inplace=True), a.check(ts, inplace=True)
        unchanged(a, pos, start)
        t = 0.0
        for k in range(3):
            t = t + TASK_DT
            p = paths[k] if poison is None else poisoned(paths[k], B, poison)
            pos = put(a, p)
            gv, reward = a.view((2, B), torch.float64, "cuda"), a.view((B,), torch.float64, "cuda")
            call(L, "riab_task_world_goal_vector", env_s, task_s, L.ptr(ts), L.ptr(world), L.ptr(pos[0]), L.ptr(pos[1]), B, 0.0,
                 L.ptr(gv[0]), L.ptr(gv[1]), stream)
            out[f"gv{k}"] = a.check(gv)
            call(L, "riab_task_world_step", env_s, task_s, L.ptr(ts), L.ptr(world), L.ptr(pos[0]), L.ptr(pos[1]), B, t, L.ptr(reward),
                 L.ptr(terminal), L.ptr(met), L.ptr(cand), L.ptr(ctl), L.ptr(diag), stream)
            out[f"reward{k}"], out[f"terminal{k}"] = a.check(reward), a.check(terminal, inplace=True)
            out[f"ts{k}"], out[f"world{k}"] = a.check(ts, inplace=True), a.check(world, inplace=True)
            a.check(met, inplace=True)
            a.check(cand, inplace=True)
            assert a.check(ctl, inplace=True).tolist() == [0, 0]
            unchanged(a, pos, p)
        gv = a.view((2, B), torch.float64, "cuda")
        call(L, "riab_task_world_reset", env_s, task_s, L.ptr(ts), L.ptr(world), B, TASK_ID0, t, n_sel, 0, TASK_SEED, 2, 0, None,
             None, L.ptr(pos[0]), L.ptr(pos[1]), None, None, L.ptr(ep_log), EP_CAP, L.ptr(ep_count), 0, 0.0, L.ptr(gv[0]),
             L.ptr(gv[1]), L.ptr(diag), stream)
        out["gv_reset"], out["world_end"], out["ts_end"] = a.check(gv), a.check(world, inplace=True), a.check(ts, inplace=True)
        again = a.view((2, B), torch.float64, "cuda")
        call(L, "riab_task_world_goal_vector", env_s, task_s, L.ptr(ts), L.ptr(world), L.ptr(pos[0]), L.ptr(pos[1]), B, 0.0,
             L.ptr(again[0]), L.ptr(again[1]), stream)
        np.testing.assert_array_equal(bits(a.check(again)), bits(out["gv_reset"]))
        out["ep_log"], out["ep_count"], out["diag"] = a.check(ep_log, inplace=True), a.check(ep_count, inplace=True), a.check(diag, inplace=True)
        unchanged(a, pos, p)
        for v, x in tables:
            unchanged(a, v, x)
        return out

    first, second = run("nan"), run("finite")
    for key in first:
        np.testing.assert_array_equal(bits(first[key]), bits(second[key]), err_msg=f"{key}: canary-dependent")
    table = first["table"]
    w = first["world_reset"]
    assert w[L.TW_N_GOALS] == n_sel and w[L.TW_GOAL_LIST:L.TW_GOAL_LIST + n_sel].astype(int).tolist() == sel
    W = orc.TaskWorld(orc.EnvSpec(walls=TASK_WALLS), table, B, goalorder, TASK_DELAY)
    W.reset(0.0, sel)
    t, awards = 0.0, 0
    for k in range(3):
        t = t + TASK_DT
        pos = paths[k][:, :B].T
        for b in range(B):
            want = goal_vector_reference(pos[b], W.goal_list, table, sequential)
            if want is not None:
                np.testing.assert_allclose(first[f"gv{k}"][:, b], want, rtol=1e-12, atol=1e-15, err_msg=f"step {k} agent {b}")
        n_before = sum(len(x.rewards) for x in W.lanes)
        totals, wterm = W.step(pos, t)
        awards += max(sum(len(x.rewards) for x in W.lanes) - n_before, 0)
        assert np.array_equal(first[f"reward{k}"], totals), (k, np.nonzero(first[f"reward{k}"] != totals))
        assert (first[f"terminal{k}"] == wterm).all(), k
        wk = first[f"world{k}"]
        assert wk[L.TW_GOAL_LIST:L.TW_GOAL_LIST + len(W.goal_list)].astype(int).tolist() == list(W.goal_list) and \
            wk[L.TW_N_GOALS] == len(W.goal_list), (k, W.goal_list)
        np.testing.assert_array_equal(first[f"ts{k}"][L.TS_N_REWARDS], [len(x.rewards) for x in W.lanes])
    assert awards >= 2, "agent 0 and the last agent each took a goal"
    assert W.lanes[0].rewards and W.lanes[B - 1].rewards and not W.lanes[1].rewards      # the first in agent order got it
    assert wterm and first["terminal2"].all() and not first["terminal1"].any()          # the flag changed at the third step
    sel2 = orc.task_reset_draws(TASK_SEED, 2, 0xFFFFFFFF, n_pool, n_sel)
    W.reset(t, sel2)
    we = first["world_end"]
    assert we[L.TW_GOAL_LIST:L.TW_GOAL_LIST + n_sel].astype(int).tolist() == sel2 and we[L.TW_EPISODE] == W.episode == 2
    assert int(first["ep_count"][0]) == 1 and first["diag"][L.TD_RESETS] == 2 and first["diag"][L.TD_REWARD_OVERFLOW] == 0
    np.testing.assert_array_equal(first["ep_log"][0], [-1.0, 1.0, 0.0, t, t])
    for b in range(B):
        want = goal_vector_reference(paths[2][:, b], W.goal_list, table, sequential)
        np.testing.assert_allclose(first["gv_reset"][:, b], want, rtol=1e-12, atol=1e-15)
    if Bp > B:
        for value in POISON:
            got = run("nan", poison=value)
            for key in first:
                np.testing.assert_array_equal(bits(got[key]), bits(first[key]), err_msg=f"{key} with {value} behind agent B")
