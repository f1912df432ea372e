// What a riab_simulate call DECIDES before it launches anything (riab_simulate.hip issues it; DESIGN.md 3.8 has the table):
// the mode, the form of the rate stage, the residency of the two kernels, the timing events it needs.  HIP-free text: the
// library compiles it, and tests/native/simulate_logic_host.cpp builds it for the host with g++ (tests/test_simulate_logic_cpu.py).
// Every input is a plain value in SimFacts, every outcome a field of SimDecision; the functions are pure.
#ifndef RIAB_SIMULATE_LOGIC_H
#define RIAB_SIMULATE_LOGIC_H

#include <cstddef>
#include <vector>

#include "riab_hip.h"

namespace riab {

struct SimPop {
  int32_t kind, n;
  bool spikes;            // spikes_base != NULL
  bool stream_supported;  // riab::stream_supported(env, pop, B) == RIAB_OK: the row-following kernel can serve it
};

struct SimFacts {
  // the call
  int32_t T, n_pops;
  int64_t B;
  uint64_t step0;
  bool forced, capturing;  // forced_pos given; the caller's stream is being captured
  int32_t timed_pop, timing_mode;
  const SimPop* pops;
  // the streamer: its options, what it has, what earlier calls left
  int strict_opt, gate_mode, side_mode, poll_max, head_rows;
  bool has_side_own, calibrated, resync, captured_once;
  int64_t step_ns_cfg, step_ns_meas, lead_mbps_cfg, lead_mbps_meas;
  bool progress_valid, same_ctrl, same_stream;  // prev_ctrl == ctrl; the earlier call's second stream was made for this stream
  uint32_t progress_end;
  size_t pairs;  // timing events it holds
  // the room
  int32_t n_walls, polygon, periodic;
  uint64_t hole_mask;
  // what only the device / the runtime can say (filled in by the caller between the two steps of the decision)
  bool idle;          // hipStreamQuery of the caller's stream; never asked, and never read, in a strict call
  bool reservable;    // the dry run of the row-following kernel in its reserving shape
  bool side_differs;  // the trajectory kernel's stream is not the caller's stream
};

struct SimDecision {
  int rc;       // RIAB_EUNSUPPORTED: strict without the streamer's own stream (riab_streamer_warmup makes it)
  bool strict;
  int form;     // RIAB_FORM_*
  int lead;     // the population whose kernel follows the trajectory row by row (-1: none); choose_lead: the candidate
  int32_t head; // rows the row-following kernel serves
  bool pure;    // exactly one kernel: device stamps / launch events time it
  int64_t lead_row_bytes;         // the candidate's bytes per row ...
  double row_ns, margin, step_ns; // ... what they take, against `margin` x a trajectory step (several populations only)
  std::vector<int32_t> sched;     // chunk form: rows per chunk
  bool timing;          // the timed population is timed (false: none asked for, a capture, a strict call short of events)
  size_t pairs_needed;  // events that takes
  // residency (decide_residency)
  bool idle, side_differs;  // the facts as the call may read them (idle: false in a strict call)
  bool open, fork, monotonic, quiet, reserve, gate, events, stamps;
  bool resync_next;  // the streamer's `resync` after an opening kernel: what the NEXT call reads as SimFacts.resync
  uint32_t serial_rows;
};

// ---- the mode ---------------------------------------------------------------------------------------------------------
// Two modes (riab_hip.h).  STRICT — asked for (RIAB_STREAMER_OPT_STRICT) or imposed by a stream that is being captured —
// allocates nothing, synchronises nothing, queries nothing and touches nothing outside this streamer: its own second
// stream (riab_streamer_warmup), an opening kernel that re-bases the control words, the two streams joined by the
// streamer's events at both ends, the started gate always.  (The check comes first: a capturing stream must not be
// queried by anything below.)
// (RIAB_STREAMER_OPT_STRICT = 2, the default: strict for runs of more than 256 steps — where its two extra launches are
// 0.2 % of the call [MI355X, cfg 2, 1024 steps: 1.423 against 1.426 G agent-steps/s] — once riab_streamer_warmup has made
// the streamer's own stream; the mode tuned for one short call per synchronisation otherwise: 846 against 1016 M at the
// 20 steps of the driver's command)
// (a call with several populations chooses its form from a step time the DEFAULT mode measures once per streamer —
// calibrate_from_stamps —: until that has happened such a call stays in the default mode)
inline void decide_mode(const SimFacts& f, SimDecision& d) {
  d.strict = f.strict_opt == 1 || f.capturing ||
             (f.strict_opt == 2 && f.T > 256 && f.has_side_own && (f.n_pops <= 1 || f.calibrated || f.step_ns_cfg != 0));
  d.rc = (d.strict && !f.has_side_own) ? RIAB_EUNSUPPORTED : RIAB_OK;  // (nothing was launched)
  d.timing = f.timed_pop >= 0 && f.timed_pop < f.n_pops && !f.capturing;  // (no timing events inside a capture)
}

// ---- what the choice "populations form or chunk form" compares ----------------------------------------------------------
// The lead's stores of a row must take at least 1.5 x as long as a trajectory step next to it, or the row-following
// kernel sits waiting for rows while nothing else runs.  Built-in figures [MI355X]: a trajectory step takes 0.9 us in
// an open room + 0.25 us per further wall (cfg 2 / cfg 5 next to their rate stage: 0.85-1.1 us, cfg 3's nine walls
// 2.05); a store-bound population writes 6.5 TB/s.  They are the fallback: the streamer MEASURES both on the chip it
// runs on from the device-clock stamps every call leaves in its control block (trajectory workgroup 0's start / last
// publication; the row-following kernel's first-wave start / last-wave end) — read once, by the first call with
// several populations that finds the caller's stream idle (the earlier call is then known to have finished), and kept
// as a factor on the built-in step time (rooms differ in walls, chips in clocks).
inline double builtin_step_ns(int n_walls) { return 900.0 + 250.0 * (n_walls > 4 ? n_walls - 4 : 0); }

inline double step_ns_now(int64_t step_ns_cfg, int64_t step_ns_meas, int n_walls) {
  if (step_ns_cfg) return (double)step_ns_cfg;
  const double b = builtin_step_ns(n_walls);
  return step_ns_meas ? b * (double)step_ns_meas / 1000.0 : b;
}
inline double lead_mbps_now(int64_t lead_mbps_cfg, int64_t lead_mbps_meas) {
  return lead_mbps_cfg ? (double)lead_mbps_cfg : (lead_mbps_meas ? (double)lead_mbps_meas : 6.5e6);
}

inline int64_t row_bytes(const SimPop& p, int64_t B) { return (int64_t)p.n * B * (p.spikes ? 5 : 4); }

// `lead`: the population whose kernel follows the trajectory row by row (rate_kernel_gated: store-bound cells without
// OU noise, whole 256-agent groups).  Alone it is the one-kernel form.  With other populations beside it, it runs
// first — when it ends every row has been published — and the others follow as their ordinary kernels over the whole
// run, in list order (a layer's inputs are earlier entries, or the lead): no gate and launch boundary per chunk, no
// short first chunks (bvc_kernel: 22 us per row in a 16-row chunk, 16.7 in a 104-row one [MI355X, cfg 3]).  That
// needs the lead's stores of a row (at 6.5 TB/s) to take at least as long as a step of the trajectory kernel next to
// it (0.9 us in an open room, + 0.25 us per further wall, x 1.5 next to a kernel that saturates HBM [MI355X: cfg 2 /
// cfg 5 0.85-1.1 us per step, cfg 3's nine walls 2.05]); otherwise its waves would sit waiting for rows while nothing
// else runs, and the chunk form keeps the trajectory hidden behind ALL the populations' work.  [MI355X, 1024 steps:
// cfg 5 158-161 -> 167-168 M agent-steps/s, bvc_kernel 38.4 -> 33.8 ms; cfg 3 (16.8 MB of GridCells per row against
// nine walls) would lose 3 % and keeps the chunks.]
// choose_lead names the CANDIDATE (alone: the population if the kernel can serve it; among several: the largest one it can
// serve that is no feed-forward layer); decide_form accepts or drops it.
inline void choose_lead(const SimFacts& f, SimDecision& d) {
  d.lead = -1;
  d.lead_row_bytes = 0;
  if (f.n_pops <= 0 || f.forced || f.T > f.poll_max) return;
  if (f.n_pops == 1) {
    if (f.pops[0].stream_supported) {
      d.lead = 0;
      d.lead_row_bytes = row_bytes(f.pops[0], f.B);
    }
  } else {
    for (int i = 0; i < f.n_pops; ++i) {
      const int64_t bytes = row_bytes(f.pops[i], f.B);
      if (f.pops[i].kind != RIAB_POP_FF && bytes > d.lead_row_bytes && f.pops[i].stream_supported) {
        d.lead_row_bytes = bytes;
        d.lead = i;
      }
    }
  }
}

// (the lead's stores of a row against 1.5 trajectory steps: measured on this chip once an earlier call's stamps can
// be read without waiting — the caller's stream is idle —, the MI355X constants until then: builtin_step_ns)
// (never in strict mode; and only when the earlier call ran on THIS stream: its idleness then says that call is over)
// True: the caller queries its stream and, if that is idle, reads the stamps (calibrate_from_stamps) before decide_form.
inline bool calibration_due(const SimFacts& f, const SimDecision& d) {
  return f.n_pops > 1 && d.lead >= 0 && !d.strict && !f.calibrated && f.step_ns_cfg == 0 && f.same_stream;
}

// chunks of rows of the chunk form: a chunk should be finished by the trajectory when the stream gets to its gate.  In a
// solid rectangular room the trajectory pulls away from the rate kernels (which need ~2.7 us per row at cfg 2) and a
// chunk may be ~1.5x its predecessor; in other rooms ~1.25x is the most (a 16, 16, 32, 64, 128 ramp then spent 230 us
// of a 1024-step run inside the gates [MI355X, rocprofv3 trace]).  Larger chunks are cheaper per row (3.6 us at 16
// rows, 2.7 at 128) and every chunk costs a gate (~5 us).
inline std::vector<int32_t> chunk_schedule(const SimFacts& env, int32_t T) {
  const bool box_room = !env.polygon && !env.hole_mask && !env.periodic && env.n_walls >= 4;
  static const int32_t ramp_fast[5] = {16, 28, 44, 64, 96};
  static const int32_t ramp_slow[10] = {16, 16, 20, 24, 32, 40, 48, 64, 80, 96};
  std::vector<int32_t> sched;
  for (int32_t t0 = 0, k = 0; t0 < T; ++k) {
    int32_t tc = box_room ? (k < 5 ? ramp_fast[k] : 128) : (k < 10 ? ramp_slow[k] : 128);
    if (tc > T - t0 || T - t0 - tc < 32) tc = T - t0;  // (no sliver at the end)
    sched.push_back(tc);
    t0 += tc;
  }
  return sched;
}

constexpr int32_t SIM_TAIL_PIECE = 512;   // head + pieces: rows per ordinary launch of the lead behind its progress gate
constexpr int32_t SIM_REST_PIECE = 1024;  // rows per launch of another population (their kernels' grids, the noise pass's loop)
constexpr int32_t SIM_SERIAL_PIECE = 4096;  // forced positions: (time rows are a grid axis of the rate kernels)

// events the timed population's launches take: start / stop of the one kernel when HIP events time it (device stamps need
// none); with a lead beside other populations or pieces, a pair for the lead and one per launch of another population;
// chunk form: a pair per chunk
inline size_t pairs_needed(const SimFacts& f, const SimDecision& d) {
  if (!d.timing) return 0;
  if (d.pure) return f.timing_mode == RIAB_TIMING_EVENTS ? 2 : 0;
  if (d.lead >= 0) return 2 * (size_t)(1 + (f.T + SIM_REST_PIECE - 1) / SIM_REST_PIECE);
  return 2 * d.sched.size();
}

// ---- which form of the rate stage (after choose_lead, and after the calibration it may have asked for) ------------------
inline void decide_form(const SimFacts& f, SimDecision& d) {
  d.head = 0;
  d.pure = false;
  d.pairs_needed = 0;
  d.row_ns = d.margin = d.step_ns = 0.0;
  d.sched.clear();
  if (f.n_pops <= 0 || f.forced) {  // the trajectory alone / kernel after kernel on one stream: nothing is timed
    d.form = f.n_pops <= 0 ? RIAB_FORM_NONE : RIAB_FORM_SERIAL;
    d.lead = -1;
    return;
  }
  if (d.lead >= 0 && f.n_pops > 1) {
    d.row_ns = (double)d.lead_row_bytes / lead_mbps_now(f.lead_mbps_cfg, f.lead_mbps_meas) * 1e3;  // bytes / (MB/s) = us; x 1e3 = ns
    // x 1.5: next to a kernel that saturates HBM the trajectory kernel's clock and its write-throughs slow down by that
    // much (cfg 2 / cfg 5: 0.85-1.1 us per step measured next to the stores against the formula's 1.35; cfg 3: 2.05
    // against 3.2).  x 2 for a MEASURED step: it was taken next to whatever the earlier call ran — in the chunk form
    // the arithmetic-bound boundary-vector kernel, which slows the trajectory less than a store stream does — and
    // includes a short call's start-up [MI355X: cfg 3's 32-step warm-up gives 1.6 us per step, not 2.05].
    d.margin = (f.step_ns_cfg == 0 && f.step_ns_meas != 0) ? 2.0 : 1.5;
    d.step_ns = step_ns_now(f.step_ns_cfg, f.step_ns_meas, f.n_walls);
    if (d.row_ns < d.margin * d.step_ns) d.lead = -1;
  }
  // Very long runs (more than 2048 rows): the row-following kernel serves the first `head_rows` rows — by then the
  // trajectory kernel (0.8-1.1 us per step) is far ahead of the rate stage (2.5 us per row at cfg 2) — and the rest of
  // the lead's rows go through its ordinary kernel, `tail_piece` rows per launch behind a progress gate that the
  // trajectory has long passed: no poll and no agent-scope position loads per workgroup.  [MI355X, cfg 2, all rows by
  // the row-following kernel vs head + pieces: 1024 steps 1.38-1.40 vs 1.37 G agent-steps/s, 2048 level, 3072 1.39-1.41
  // vs 1.45, 4096 1.34-1.38 vs 1.43-1.46, 8192 1.38-1.44 vs 1.49; cfg 4 at 1024 steps 0.37-0.39 vs 0.36 G.]
  d.head = d.lead < 0 ? 0 : ((f.T <= 2048 || f.T <= f.head_rows) ? f.T : f.head_rows);
  d.pure = d.lead >= 0 && f.n_pops == 1 && d.head == f.T;
  d.form = d.lead < 0 ? RIAB_FORM_CHUNKS
                      : (f.n_pops > 1 ? RIAB_FORM_POPULATIONS : (d.pure ? RIAB_FORM_ONE_KERNEL : RIAB_FORM_HEAD_AND_PIECES));
  if (d.lead < 0) {
    d.lead_row_bytes = 0;
    d.sched = chunk_schedule(f, f.T);
  }
  // (a strict call creates nothing: it is timed with the events riab_streamer_warmup made, or not at all)
  d.pairs_needed = pairs_needed(f, d);
  if (d.strict && f.pairs < d.pairs_needed) {
    d.timing = false;
    d.pairs_needed = 0;
  }
}

// ---- residency, and the order between the two streams (once `idle`, `reservable` and `side_differs` are known) ----------
inline void decide_residency(const SimFacts& f, SimDecision& d) {
  d.idle = !d.strict && f.idle;
  d.side_differs = f.side_differs;
  // The opening kernel: a strict call re-bases the announcement counter and this call's progress words on the device, so
  // that a replay of the captured call finds what the first run found; once that has happened, the host's mirror of the
  // counter means nothing any more and the next call of either mode re-bases as well.
  d.open = d.strict || f.resync;
  // (a default-mode call has re-based: its successors count on from here — unless a strict call has ever been CAPTURED:
  // it may be replayed any time, and every later call opens)
  d.resync_next = d.open && (d.strict || f.captured_once || f.capturing);
  // The trajectory kernel has to start after what the caller's stream holds (earlier calls' kernels wrote the state it
  // reads).  When that stream is idle — the case that matters for latency: one short call per synchronisation — there is
  // nothing to wait for and the launch goes out with no API call in front of it but the query; otherwise an event carries
  // the order.
  d.fork = (!d.idle || d.open) && d.side_differs;
  // Progress words hold absolute step counts and every trajectory workgroup resets its own to step0 before it
  // announces itself.  A call that starts at or beyond the end of the last call on this block can never meet a word
  // above its own rows; any other call (the same block replayed, another ctrl block) must not let a consumer look at
  // the words before every workgroup has announced itself: it takes the started gate.
  d.monotonic = f.progress_valid && f.same_ctrl && (int32_t)((uint32_t)f.step0 - f.progress_end) >= 0;
  // Both kernels must be resident at once or the rate waves spin for nothing (riab_hip.h "Residency"): either the
  // row-following kernel is launched in its reserving shape — twelve-wave workgroups, one wave slot per SIMD always
  // free for a trajectory workgroup: no gate — or a one-wave gate in front of it returns only once every trajectory
  // workgroup of THIS launch has announced itself: the rate waves can then never occupy the slots the kernel they wait
  // for still needs, whatever else runs on the device (another stream, another process: two ranks sharing one GPU ran
  // into the waits' time limit with neither).  RIAB_GATE_WHEN_BUSY drops both when the caller's stream was idle.
  d.events = d.pure && d.timing && f.timed_pop == d.lead && f.timing_mode == RIAB_TIMING_EVENTS;
  // (device-clock stamps of the row-following kernel: one store by the grid's first wave, one maximum by the sixteen
  // waves of the last row's last cell group — always on unless HIP events time the launch; they need no reset: the
  // clock only moves forward)
  d.stamps = !d.events;
  // residency (riab_hip.h): the reserving shape of the row-following kernel needs no gate; everything else takes one —
  // unless the caller has said that it owns the device (RIAB_GATE_WHEN_BUSY) and its stream is idle
  d.quiet = d.idle && !d.open && d.pure && d.monotonic && d.side_differs;
  // (the reserving shape is only offered by kernels whose registers leave a trajectory workgroup room: launch_stream_cell)
  d.reserve = d.quiet && f.gate_mode == RIAB_GATE_RESERVED && f.reservable;
  // (the chunk form has no started gate: its first progress gate also waits until every trajectory workgroup is resident)
  d.gate = d.lead >= 0 && !(d.reserve || (d.quiet && f.gate_mode == RIAB_GATE_WHEN_BUSY)) && d.side_differs;
  d.serial_rows = f.T >= 8 ? (uint32_t)f.T : 0u;
}

// The caller's stream continues after the trajectory kernel as well (its state rows, its last history rows).  Every
// form above ends with a kernel on the caller's stream that has waited for the trajectory kernel's LAST publication,
// and the four-wave kernel makes that publication after its state stores have been written through (t4_store_state):
// the stream order of the caller's stream already carries the dependency.  An event between the streams is only
// needed for the two-wave kernel (RIAB_OPT_TRAJ_KERNEL = 2) — and after a failure, when nothing may have waited.
// [MI355X, cfg 2, 20 steps: the event's record + wait were 4.7 us of host time and its barrier packet sat between the
// rate kernel's end and the host's wake-up: 97 -> 89 us per call without them.]
// When the caller's stream was BUSY at the call, host time is not what the call is short of: the event is recorded as
// well — should a wait of the rate stage give up (abort flag), whatever follows on the caller's stream is then still
// ordered behind the trajectory kernel.  (After an abort on an idle stream the host layer synchronises the device
// before it clears the flags: Agent._check_pipeline.)
inline bool needs_join(const SimDecision& d, bool state_published, bool fail) {
  return (!state_published || fail || !d.idle || d.open) && d.side_differs;
}

// Kernel launches of a call in which no launch fails: what riab_streamer_info(3) reports after it.  Three quirks, kept
// as they are (tests pin the numbers): 0, not 1 + the populations' launches, after a forced-positions call; the populations
// form does not count the OTHER populations' launches; the chunk form counts 1 + n_pops per chunk it gets to, also for a
// chunk whose gate or kernels failed to launch.
inline int planned_launches(const SimFacts& f, const SimDecision& d) {
  if (f.n_pops <= 0) return 1;
  if (f.forced) return 0;
  const int traj = d.open ? 2 : 1;
  if (d.lead < 0) return traj + (1 + f.n_pops) * (int)d.sched.size();
  return traj + (d.gate ? 1 : 0) + 1 + 2 * ((f.T - d.head + SIM_TAIL_PIECE - 1) / SIM_TAIL_PIECE);
}

}  // namespace riab
#endif
