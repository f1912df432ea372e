// The open-loop path as ONE native call (include/riab_hip.h: riab_simulate): the trajectory kernel and the
// firing-rate stage run CONCURRENTLY on two streams, coupled by flags in device memory.  This file is host code only:
// the kernels live in riab_traj4_kernel.h (the publishing trajectory kernel: rows written through + progress words)
// and riab_rates.hip (rate_kernel_gated, stream_gate_kernel, and every population's ordinary kernel).
//
// Why not one launch: a launch has ONE register and LDS allocation.  The trajectory kernel needs 220 VGPRs and 80 KB
// of LDS per 64 agents; the rate kernels need ~40 VGPRs and no LDS and live on occupancy.  Why not launches per chunk
// behind HIP events: every chunk pays the fill of the first stage and a dependent launch boundary, and a 20-step run
// has nothing to overlap.  With flags the rate stage starts a step or two behind the trajectory and stays there.
//
// Which stream carries what.  The rate stage ends last, so IT runs on the caller's stream and the trajectory kernel on
// the streamer's own: the join (caller's stream waits for the trajectory kernel) is then a barrier whose dependency was
// met tens of microseconds before the rate stage finishes, and a host synchronisation returns as soon after the last
// kernel as after any single kernel (~10 us).  The other way round — rate stage on the second stream, round 2 — the
// join sat behind the LAST kernel: its signal had to travel second queue -> event -> barrier packet on the first
// queue -> host, 25 us from the end of the rate kernel to the return of hipDeviceSynchronize [MI355X, rocprofv3
// --hip-trace --kernel-trace of the driver's bench command].
//
// Two forms of the rate stage:
//  * one store-bound population (place / grid / head-direction cells without OU noise), up to `poll_max` steps
//    (default 65535, the grid's limit): ONE rate kernel for all rows whose waves wait for their rows themselves
//    (rate_kernel_gated, nontemporal stores).  Workgroups are dispatched in row order, so the resident ones are always
//    the oldest unfinished rows — the ones at or behind the trajectory's frontier.
//  * anything else: per chunk of rows (16, 28, 44, ... 128) a one-wave progress gate, then every population's ordinary
//    kernel over the chunk in list order, at the price of a chunk of distance to the trajectory and a gate + launch
//    boundary (~5 us) per chunk.
//    Until round 3 the first form was limited to 256 steps: with the single-wave trajectory kernel (2.6 us per step,
//    slower than most rate kernels) and ordinary stores the chunk form was ahead beyond that.  With the four-wave
//    trajectory kernel and nontemporal stores the one-kernel form is level or ahead at every length and population
//    size measured [MI355X, tools/form_probe.py, 4096 agents, 1024 / 4096 steps: n = 64: 5.0 / 5.5 G agent-steps/s in
//    both forms; n = 384: 3.47 vs 2.57 G; n = 1024: 1.36 vs 1.15 G at 1024 steps, level at 4096].
//    A PERSISTENT rate kernel was built first (three versions) and removed: waves that stay resident hold store credits
//    and lose 9-12 % of the store bandwidth against freshly dispatched ones (tools/stream_bench.hip).
// Forced (imported) trajectories have no recurrence to hide: their kernel and the populations' kernels simply follow
// each other on the caller's stream.
#include <hip/hip_ext.h>

#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "riab_agent_kernel.h"
#include "riab_launch.h"
#include "riab_simulate_logic.h"

struct RiabStreamer {
  hipStream_t side = nullptr;  // the trajectory kernel's stream (SIDE_STREAM 0): BORROWED from the process-wide pool of screened
                               // streams (side_stream_for), for the caller's stream `side_main`; `side_screened`: it has been timed
  hipStream_t side_main = nullptr;
  bool side_screened = false;
  int dev = 0;
  int side_pair_ns = 0, side_ref_ns = 0, side_rejected = 0;   // what the screening measured (riab_streamer_info 4 / 5 / 6)
  hipStream_t side_normal = nullptr;  // ... at the default priority (created when RIAB_STREAMER_OPT_SIDE_STREAM = 1 is first used)
  int side_mode = 0;           // RIAB_STREAMER_OPT_SIDE_STREAM
  // form selection (populations form against chunk form): a trajectory step next to the rate stage / the lead's store rate
  int64_t step_ns_cfg = 0, lead_mbps_cfg = 0;    // configured (0: measure)
  int64_t step_ns_meas = 0, lead_mbps_meas = 0;  // measured from the stamps of an earlier call (0: not yet)
  bool calibrated = false;                       // the one blocking read of the stamps has been made (or given up)
  // what the last call left for that measurement: its ctrl block, rows, walls, the lead's bytes per row (0: no lead)
  uint32_t* prev_ctrl = nullptr;
  int32_t prev_T = 0, prev_walls = 0;
  int64_t prev_lead_row_bytes = 0;
  uint32_t progress_end = 0;   // (uint32) step0 + T of the last call on prev_ctrl: a later call must start at or beyond it
  bool progress_valid = false;
  int last_launches = 0;       // kernel launches of the last call (riab_simulate_logic.h: planned_launches, and its quirks)
  int64_t late_calls = 0;      // calls whose rate stage the HOST launched late (> 12 us after the trajectory kernel's launch had
                               // returned: a descheduled thread, a kernel's first launch): such a call can find every row
                               // published without any hardware queue being shared — the RIAB_CTRL_SERIALISED count is read
                               // against this one (riab_streamer_info 7)
  hipEvent_t fork = nullptr, join = nullptr;  // caller's stream -> side (only when the caller's stream is busy), side -> caller's stream
  std::vector<hipEvent_t> pairs;  // timing events (created on first use): (start, stop) around every launch of the timed population;
                                  // the first pair around the rate kernel of a one-kernel call timed by HIP events
  int n_pairs = 0;             // pairs recorded by the last call (0: the first pair or the device stamps hold the measurement)
  int timed = 0;               // 0 nothing, 1 events, 2 device time stamps (ctrl[RIAB_CTRL_STAMPS])
  uint32_t* stamp_ctrl = nullptr;  // control block of the last stamped call
  uint32_t started_total = 0;  // trajectory workgroups launched so far through this object (wraps like the device word)
  int wall_khz = 100000;       // rate of the device's constant clock (s_memrealtime)
  int gate_mode = RIAB_GATE_RESERVED;  // RIAB_STREAMER_OPT_GATE
  int poll_max = 65535;        // RIAB_STREAMER_OPT_POLL_MAX
  int head_rows = 256;         // RIAB_STREAMER_OPT_HEAD_ROWS
  int last_form = RIAB_FORM_NONE;  // riab_streamer_last_form
  // the strict mode (riab_hip.h "Two modes")
  int strict = 2;              // RIAB_STREAMER_OPT_STRICT
  hipStream_t side_own = nullptr;  // the trajectory kernel's stream in strict calls: the streamer's own, made by riab_streamer_warmup
  bool resync = false;         // a strict call has re-based the announcement counter: the next call of either mode opens with
                               // stream_open_kernel as well
  bool captured_once = false;  // ... and every later call does, once a strict call has been CAPTURED (it may be replayed any time)
  uint32_t spin_limit = 0u;    // RIAB_STREAMER_OPT_SPIN_LIMIT: polls before a waiting wave / gate gives up (0: the defaults)
  int last_strict = 0;         // the last call ran in strict mode (riab_streamer_info 8)
};

// ---- the trajectory kernel's stream: screened, process-wide -----------------------------------------------------------
// Not every HIP stream is as good as the next.  The runtime multiplexes a process's streams onto a few hardware queues
// (GPU_MAX_HW_QUEUES), and a stream that lands on the CALLER's queue costs every pair of launches on the two streams
// ~50 us: tools/queue_probe.hip — a tiny kernel on the null stream + one on the new stream + synchronise: 21 us on most
// streams, 52-75 us on every third or fourth one created; simulate(20) at the bench shape then takes 124 us instead
// of 80 although its kernels overlap on the device as usual (tools/slow_mode_probe.py) [MI355X, ROCm 7.2].  Which streams
// are slow depends on how many the process has created and kept, at either priority.  So the second stream is not
// simply created: candidates (highest priority: queues apart from the default-priority streams' in most processes,
// DESIGN.md 7) are TIMED against the caller's stream — the same pair of launches, best of six — and the first one
// within 20 us of two launches on the caller's stream alone is kept; rejected candidates stay allocated (destroying
// one hands its queue to the next candidate).  One screened stream per (device, caller's stream) for the whole process:
// every streamer of that caller borrows it (calls on one caller's stream are ordered anyway).  Screening needs the
// caller's stream idle (it synchronises it); a first call that finds it busy borrows an unscreened stream and the
// screening happens at the first idle call.
// The pool is BOUNDED: at most SIDE_POOL_CAP caller streams per device have an entry.  One more caller's stream takes over
// the least recently used entry with its stream (unscreened for the new pair; a streamer still holding that stream for
// its old caller keeps working: a HIP stream shared by two callers is still an ordered queue, the two only queue behind
// each other there), and once PARKED_CAP rejected candidates are parked they are tried again for other callers instead of
// creating more.  A process that makes a new torch stream per task therefore holds a few dozen HIP streams, not six per
// stream it ever used.
namespace {
constexpr size_t SIDE_POOL_CAP = 8, PARKED_CAP = 24;
struct SideEntry {
  int dev;
  hipStream_t main, side;
  bool screened;
  int pair_ns, ref_ns, rejected;
  uint64_t last_use;
};
uint64_t g_side_tick = 0;
std::mutex g_side_mu;
std::vector<SideEntry> g_side;
std::vector<hipStream_t> g_parked;  // rejected candidates: kept for the life of the process
uint32_t* g_scratch[64] = {nullptr};

double host_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// a one-wave kernel that returns at once (started_target 0 against zeroed words)
void tiny_launch(uint32_t* scratch, hipStream_t s) { (void)riab::launch_stream_gate(scratch, 0u, 0u, 0u, 1u, false, 0u, s); }

// best of `n`: [one launch on `a`, one on `b`, synchronise both], microseconds
double pair_us(uint32_t* scratch, hipStream_t a, hipStream_t b, int n) {
  double best = 1e30;
  for (int k = 0; k < n + 2; ++k) {
    const double t0 = host_us();
    tiny_launch(scratch, a);
    tiny_launch(scratch, b);
    (void)hipStreamSynchronize(b);
    (void)hipStreamSynchronize(a);
    const double t = host_us() - t0;
    if (k >= 2 && t < best) best = t;  // (two warm-up rounds: a stream's first launches set its queue up)
  }
  return best;
}

hipStream_t new_candidate() {
  if (g_parked.size() >= PARKED_CAP) {  // (set aside for another caller's stream: may do for this one)
    hipStream_t s = g_parked.front();
    g_parked.erase(g_parked.begin());
    return s;
  }
  int least = 0, greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
  hipStream_t s = nullptr;
  if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest) != hipSuccess) return nullptr;
  return s;
}

// the screened stream for (dev, main_s); `idle`: the caller's stream is idle, screening may synchronise it
bool side_stream_for(RiabStreamer* h, hipStream_t main_s, bool idle) {
  std::lock_guard<std::mutex> lock(g_side_mu);
  SideEntry* e = nullptr;
  for (SideEntry& x : g_side)
    if (x.dev == h->dev && x.main == main_s) e = &x;
  if (!e) {
    size_t on_dev = 0;
    SideEntry* lru = nullptr;
    for (SideEntry& x : g_side) {
      if (x.dev != h->dev) continue;
      on_dev += 1;
      if (!lru || x.last_use < lru->last_use) lru = &x;
    }
    if (on_dev >= SIDE_POOL_CAP && lru) {  // bounded pool: the least recently used caller's entry, stream included
      lru->main = main_s;
      lru->screened = false;
      lru->pair_ns = lru->ref_ns = lru->rejected = 0;
      e = lru;
    } else {
      g_side.push_back(SideEntry{h->dev, main_s, nullptr, false, 0, 0, 0, 0});
      e = &g_side.back();
    }
  }
  e->last_use = ++g_side_tick;
  int cur_dev = -1;
  (void)hipGetDevice(&cur_dev);   // (screening allocates and launches on the CURRENT device: only when that is the streamer's)
  if (!e->screened && idle && cur_dev == h->dev && h->dev >= 0 && h->dev < 64) {
    uint32_t*& scratch = g_scratch[h->dev];
    if (!scratch) {
      if (hipMalloc((void**)&scratch, 256) != hipSuccess || hipMemset(scratch, 0, 256) != hipSuccess) scratch = nullptr;
    }
    if (scratch) {
      const double ref = pair_us(scratch, main_s, main_s, 6);
      hipStream_t best_s = e->side;  // (an unscreened stream borrowed by an earlier, busy call is the first candidate)
      double best = 1e30;
      int rejected = 0;
      for (int c = 0; c < 6; ++c) {
        hipStream_t cand = (c == 0 && e->side) ? e->side : new_candidate();
        if (!cand) break;
        const double t = pair_us(scratch, main_s, cand, 6);
        if (t < best) {
          if (best_s && best_s != cand) g_parked.push_back(best_s);
          best = t;
          best_s = cand;
        } else {
          g_parked.push_back(cand);
        }
        if (t <= ref + 20.0) break;
        ++rejected;
      }
      if (best_s) {
        e->side = best_s;
        e->screened = true;
        e->pair_ns = (int)(best * 1e3);
        e->ref_ns = (int)(ref * 1e3);
        e->rejected = rejected;
      }
    }
  }
  if (!e->side) e->side = new_candidate();
  if (!e->side) return false;
  h->side = e->side;
  h->side_main = main_s;
  h->side_screened = e->screened;
  h->side_pair_ns = e->pair_ns;
  h->side_ref_ns = e->ref_ns;
  h->side_rejected = e->rejected;
  return true;
}
}  // namespace

extern "C" RiabStreamer* riab_streamer_create(void) {
  RiabStreamer* h = new (std::nothrow) RiabStreamer();
  if (!h) return nullptr;
  int khz = 0;
  if (hipGetDevice(&h->dev) != hipSuccess || hipEventCreateWithFlags(&h->join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->fork, hipEventDisableTiming) != hipSuccess) {
    riab_streamer_destroy(h);
    return nullptr;
  }
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->dev) == hipSuccess && khz > 0) h->wall_khz = khz;
  return h;
}

extern "C" int riab_streamer_configure(RiabStreamer* h, int32_t option, int32_t value) {
  if (!h) return RIAB_EINVAL;
  switch (option) {
    case RIAB_STREAMER_OPT_GATE:
      if (value != RIAB_GATE_ALWAYS && value != RIAB_GATE_WHEN_BUSY && value != RIAB_GATE_RESERVED) return RIAB_EINVAL;
      h->gate_mode = value;
      return RIAB_OK;
    case RIAB_STREAMER_OPT_SIDE_STREAM:
      if (value < 0 || value > 2) return RIAB_EINVAL;
      if (value == 1 && !h->side_normal && hipStreamCreateWithFlags(&h->side_normal, hipStreamNonBlocking) != hipSuccess)
        return RIAB_EINVAL;
      h->side_mode = value;
      return RIAB_OK;
    case RIAB_STREAMER_OPT_STEP_NS:
      if (value < 0) return RIAB_EINVAL;
      h->step_ns_cfg = value;
      return RIAB_OK;
    case RIAB_STREAMER_OPT_LEAD_MBPS:
      if (value < 0) return RIAB_EINVAL;
      h->lead_mbps_cfg = value;
      return RIAB_OK;
    case RIAB_STREAMER_OPT_POLL_MAX:
      if (value < 0 || value > 65535) return RIAB_EINVAL;
      h->poll_max = value;
      return RIAB_OK;
    case RIAB_STREAMER_OPT_HEAD_ROWS:
      if (value < 1 || value > 65535) return RIAB_EINVAL;
      h->head_rows = value;
      return RIAB_OK;
    case RIAB_STREAMER_OPT_STRICT:
      if (value < 0 || value > 2) return RIAB_EINVAL;
      h->strict = value;
      return RIAB_OK;
    case RIAB_STREAMER_OPT_SPIN_LIMIT:
      if (value < 0) return RIAB_EINVAL;
      h->spin_limit = (uint32_t)value;
      return RIAB_OK;
    default: return RIAB_EINVAL;
  }
}

extern "C" void riab_streamer_destroy(RiabStreamer* h) {
  if (!h) return;
  for (hipEvent_t e : h->pairs) (void)hipEventDestroy(e);
  if (h->join) (void)hipEventDestroy(h->join);
  if (h->fork) (void)hipEventDestroy(h->fork);
  // (h->side belongs to the process-wide pool: side_stream_for)
  if (h->side_normal) (void)hipStreamDestroy(h->side_normal);
  if (h->side_own) (void)hipStreamDestroy(h->side_own);
  delete h;
}

extern "C" int riab_streamer_last_form(RiabStreamer* h) { return h ? h->last_form : RIAB_FORM_NONE; }

// the step time and the lead's store rate that the form selection compares (riab_simulate_logic.h), measured on this chip
static void calibrate_from_stamps(RiabStreamer* h) {
  if (!h->prev_ctrl || h->prev_T < 8) return;  // (nothing to read yet: try again at the next call)
  h->calibrated = true;                         // one blocking copy per streamer, not one per call
  unsigned long long st[4] = {0, 0, 0, 0};      // STAMPS (2 x u64) and TRAJ_STAMPS (2 x u64): words 8 .. 15
  static_assert(RIAB_CTRL_TRAJ_STAMPS == RIAB_CTRL_STAMPS + 4, "the two stamp pairs are read with one copy");
  if (hipMemcpy(st, h->prev_ctrl + RIAB_CTRL_STAMPS, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess) return;
  const double tick_ns = 1e6 / (double)h->wall_khz;
  if (st[3] > st[2]) {
    const double step = (double)(st[3] - st[2]) * tick_ns / (double)h->prev_T;
    if (step > 50.0 && step < 1e6) h->step_ns_meas = (int64_t)(step * 1000.0 / riab::builtin_step_ns(h->prev_walls));  // per mille
  }
  if (h->prev_lead_row_bytes > 0 && st[1] > st[0]) {
    const double ns = (double)(st[1] - st[0]) * tick_ns;
    const double mbps = (double)h->prev_lead_row_bytes * (double)h->prev_T / ns * 1e3;  // bytes / ns = GB/s; x 1e3 = MB/s
    if (mbps > 1e4 && mbps < 2e7) h->lead_mbps_meas = (int64_t)mbps;
  }
}

extern "C" int64_t riab_streamer_info(RiabStreamer* h, int32_t which) {
  if (!h) return -1;
  switch (which) {
    case 0: return (int64_t)riab::step_ns_now(h->step_ns_cfg, h->step_ns_meas, 4);
    case 1: return (int64_t)riab::lead_mbps_now(h->lead_mbps_cfg, h->lead_mbps_meas);
    case 2: return (h->step_ns_cfg == 0 && h->step_ns_meas != 0) ? 1 : 0;
    case 3: return h->last_launches;
    case 4: return h->side_screened ? h->side_pair_ns : -1;
    case 5: return h->side_rejected;
    case 6: return h->side_ref_ns;
    case 7: return h->late_calls;
    case 8: return h->last_strict;
    case 9: return h->side_own ? 1 : 0;
    case 10: {  // HIP streams the process-wide pool holds on this streamer's device (entries' + parked)
      std::lock_guard<std::mutex> lock(g_side_mu);
      int64_t n = (int64_t)g_parked.size();
      for (const SideEntry& x : g_side) n += (x.dev == h->dev && x.side) ? 1 : 0;
      return n;
    }
    default: return -1;
  }
}

extern "C" float riab_streamer_last_rate_ms(RiabStreamer* h) {
  if (!h || !h->timed) return -1.0f;
  float ms = -1.0f;
  if (h->timed == 2) {  // first wave's start / last wave's end of the gated rate kernel, on the device's constant clock
    unsigned long long st[2] = {0, 0};
    if (hipMemcpy(st, h->stamp_ctrl + RIAB_CTRL_STAMPS, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess) return -1.0f;
    if (st[1] <= st[0]) return -1.0f;
    return (float)((double)(st[1] - st[0]) / (double)h->wall_khz);
  }
  if (h->n_pairs > 0) {  // the sum over the timed population's launches of the last chunk-form call
    float total = 0.0f;
    for (int i = 0; i < h->n_pairs; ++i) {
      if (hipEventElapsedTime(&ms, h->pairs[2 * i], h->pairs[2 * i + 1]) != hipSuccess) return -1.0f;
      total += ms;
    }
    return total;
  }
  if (hipEventElapsedTime(&ms, h->pairs[0], h->pairs[1]) != hipSuccess) return -1.0f;
  return ms;
}


// ---- any set of populations: the chunked form of the rate stage for all of them, one native call ----------------
// rows [t0, t0 + tc) of population i from the trajectory rows of the same chunk: `tc` calls of Neurons.update on
// successive rows (riab_plan.hip: launch_population_rows, which says what differs from a step plan's one-row launches)
static int launch_pop_rows(const RiabSimulate* q, int i, int32_t t0, int32_t tc, hipStream_t s) {
  riab::PopRows r = {};
  r.env = q->env;
  r.pops = q->pops;
  r.index = i;
  r.hist = q->hist + (int64_t)t0 * RIAB_HIST_ROWS * q->B;
  r.hist_ld = (int64_t)RIAB_HIST_ROWS * q->B;
  r.B = q->B;
  r.T = tc;
  r.rate_row = t0;
  r.dt = (float)q->motion->dt;
  r.seed = q->seed;
  r.step0 = q->step0 + 1 + (uint64_t)t0;  // Neurons.update after the (step0 + t + 1)-th Agent.update
  r.agent_id0 = q->agent_id0;
  return riab::launch_population_rows(r, s, nullptr);
}

static int check_populations(const RiabPopulation* pops, int32_t n_pops, int32_t T) {
  for (int i = 0; i < n_pops; ++i) {
    const RiabPopulation& q = pops[i];
    if (q.n <= 0 || !q.rates_base || q.capacity_rows < T) return RIAB_EINVAL;
    // (velocity and phase-precessing cells read the float64 state: they advance through a step plan)
    if (!riab::population_kind_known(q.kind) || q.kind == RIAB_POP_VELOCITY || q.kind == RIAB_POP_THETA_PLACE)
      return RIAB_EUNSUPPORTED;
    const int rc = riab::check_population(q, i);  // (refused before the trajectory kernel is in flight, not by a chunk's launch)
    if (rc) return rc;
    if (q.kind == RIAB_POP_FF)
      for (int l = 0; l < q.n_inputs; ++l)
        if (pops[q.input_index[l]].capacity_rows < T) return RIAB_EINVAL;
  }
  return RIAB_OK;
}

extern "C" int riab_watch_compare(const RiabWatch* watch, int32_t n) {
  if (n < 0 || (n > 0 && !watch)) return RIAB_EINVAL;
  for (int32_t i = 0; i < n; ++i) {
    const RiabWatch& w = watch[i];
    if (w.bytes < 0 || (w.bytes > 0 && (!w.live || !w.snapshot))) return RIAB_EINVAL;
    if (w.bytes > 0 && memcmp(w.live, w.snapshot, (size_t)w.bytes) != 0) return RIAB_ECHANGED;
  }
  return RIAB_OK;
}

// the streamer holds `need` timing events: created here (first use) unless the call may create nothing (a strict call)
static bool ensure_pairs(RiabStreamer* h, size_t need, bool may_create) {
  while (may_create && h->pairs.size() < need) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return false;
    h->pairs.push_back(e);
  }
  return h->pairs.size() >= need;
}

// Everything riab_simulate may have to set up, done ahead of it (riab_hip.h "Two modes"): the strict mode's own second
// stream, the screening of the default mode's second stream for `stream` (which synchronises it), the events a timed
// call records.  Allocates and synchronises — that is its purpose; calls after it do neither.
extern "C" int riab_streamer_warmup(RiabStreamer* h, riab_stream_t stream) {
  if (!h) return RIAB_EINVAL;
  hipStream_t main_s = (hipStream_t)stream;
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(main_s, &capturing) == hipSuccess && capturing != hipStreamCaptureStatusNone) return RIAB_EUNSUPPORTED;
  if (!h->side_own) {
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (hipStreamCreateWithPriority(&h->side_own, hipStreamNonBlocking, greatest) != hipSuccess) {
      h->side_own = nullptr;
      return RIAB_EINVAL;
    }
  }
  if (!ensure_pairs(h, 64, true)) return RIAB_EINVAL;
  if (hipStreamSynchronize(main_s) != hipSuccess) return RIAB_EINVAL;
  if (h->side_mode == 0 && !side_stream_for(h, main_s, true)) return RIAB_EINVAL;
  return RIAB_OK;
}

// ---- riab_simulate in stages: validate, facts, decide (riab_simulate_logic.h), provision events, trajectory launch, -----
// ---- one of three issue functions, join ---------------------------------------------------------------------------------
namespace {
struct SimRun {  // one call on its way through the stages
  RiabStreamer* h;
  const RiabSimulate* q;
  riab::SimDecision d;
  hipStream_t main_s, side_s;
  uint32_t n_traj;  // trajectory workgroups
  double t_traj_launched;
  bool late_noted;
  // ~0.3 us per poll: a generous second or two before a wait gives up (a healthy wait is tens of microseconds)
  uint32_t spin_limit() const { return h->spin_limit ? h->spin_limit : 1u << 20; }
  uint32_t gate_limit(uint32_t dflt) const { return h->spin_limit ? h->spin_limit : dflt; }
  void note_first_rate_launch() {  // (after the first launch of the rate stage has returned)
    // (only calls that CAN be counted as serialised — eight rows or more — are counted as late: the two counts are
    // subtracted from each other)
    if (!late_noted && q->T >= 8 && host_us() - t_traj_launched > 12.0) ++h->late_calls;
    late_noted = true;
  }
  // the lead's row-following kernel over the head rows; a dry run checks its arguments (and whether it offers `reserve`)
  int rate_stream(bool dry_run, bool reserve) const {
    const bool ev = !dry_run && d.events;
    return riab::launch_rate_stream(q->env, &q->pops[d.lead], q->hist, q->B, d.head, (float)q->motion->dt, q->seed, q->step0,
                                    q->agent_id0, q->ctrl, spin_limit(), !dry_run && d.stamps, main_s, ev ? h->pairs[0] : nullptr,
                                    ev ? h->pairs[1] : nullptr, dry_run, reserve, dry_run ? 0u : d.serial_rows);
  }
};

// stage 1: every argument check before the first launch
int validate(const RiabStreamer* h, const RiabSimulate* q, riab::AgentArgs& a) {
  if (!h || !q || !q->env || !q->motion || !q->ctrl || !q->hist || q->n_pops < 0 || (q->n_pops > 0 && !q->pops) || q->T <= 0)
    return RIAB_EINVAL;
  if (q->B <= 0 || q->B % 4 != 0) return RIAB_EALIGN;
  if (q->forced_pos && (q->noise || q->drift)) return RIAB_EINVAL;
  // the caller's cached tables against the host arrays they were built from (RiabSimulate.watch): before anything else
  int rc = riab_watch_compare(q->watch, q->n_watch);
  if (!rc) rc = check_populations(q->pops, q->n_pops, q->T);
  if (!rc)
    rc = riab::fill_agent_args(a, q->env, q->motion, q->state, q->B, q->agent_id0, q->drift, q->noise, nullptr, q->forced_pos,
                               q->seed, q->step0, q->T, q->hist, q->diag, q->resample_pos);
  a.ctrl = q->ctrl;
  return rc;
}

// stage 2: what the decisions read, as plain values (idle, reservable, side_differs: filled in as the call learns them)
riab::SimFacts gather_facts(const RiabStreamer* h, const RiabSimulate* q, hipStream_t main_s, bool capturing,
                            std::vector<riab::SimPop>& pops) {
  riab::SimFacts f = {};
  f.T = q->T, f.n_pops = q->n_pops, f.B = q->B, f.step0 = q->step0;
  f.forced = q->forced_pos != nullptr, f.capturing = capturing;
  f.timed_pop = q->timed_pop, f.timing_mode = q->timing_mode;
  for (int i = 0; i < q->n_pops; ++i)
    pops.push_back({q->pops[i].kind, q->pops[i].n, q->pops[i].spikes_base != nullptr,
                    riab::stream_supported(q->env, &q->pops[i], q->B) == RIAB_OK});
  f.pops = pops.data();
  f.strict_opt = h->strict, f.gate_mode = h->gate_mode, f.poll_max = h->poll_max, f.head_rows = h->head_rows;
  f.has_side_own = h->side_own != nullptr, f.calibrated = h->calibrated, f.resync = h->resync, f.captured_once = h->captured_once;
  f.step_ns_cfg = h->step_ns_cfg, f.step_ns_meas = h->step_ns_meas;
  f.lead_mbps_cfg = h->lead_mbps_cfg, f.lead_mbps_meas = h->lead_mbps_meas;
  f.progress_valid = h->progress_valid, f.same_ctrl = h->prev_ctrl == q->ctrl, f.same_stream = h->side_main == main_s;
  f.progress_end = h->progress_end, f.pairs = h->pairs.size();
  f.n_walls = q->env->n_walls, f.polygon = q->env->polygon, f.periodic = q->env->periodic, f.hole_mask = q->env->hole_mask;
  return f;
}

// the trajectory kernel's stream.  (RIAB_STREAMER_OPT_SIDE_STREAM: 1 a stream at the default priority, 2 the caller's own
// stream — the two kernels then run one after the other, which is what the RIAB_CTRL_SERIALISED diagnostic is tested with)
bool second_stream(RiabStreamer* h, hipStream_t main_s, bool strict, bool idle, hipStream_t* side_s) {
  if (!strict && h->side_mode == 0 && (h->side_main != main_s || !h->side || (!h->side_screened && idle))) {
    if (!side_stream_for(h, main_s, idle)) return false;
  }
  *side_s = strict ? h->side_own
                   : (h->side_mode == 2 ? main_s : (h->side_mode == 1 && h->side_normal ? h->side_normal : h->side));
  return true;
}

// stage 5: the opening kernel and the fork if the decision has them, then the trajectory kernel on the second stream
int launch_trajectory(SimRun& r, riab::AgentArgs& a, bool capturing, bool* state_published) {
  RiabStreamer* h = r.h;
  const RiabSimulate* q = r.q;
  if (r.d.open) {
    const int rc = riab::launch_stream_open(q->ctrl, r.n_traj, (uint32_t)q->step0, r.main_s);
    if (rc) return rc;
    // MIRROR, the counter has been re-based on the device:
    h->started_total = 0;
    if (capturing) h->captured_once = true;
    h->resync = r.d.resync_next;
  }
  if (r.d.fork) {
    hipError_t e = hipEventRecord(h->fork, r.main_s);
    if (e == hipSuccess) e = hipStreamWaitEvent(r.side_s, h->fork, 0);
    if (e != hipSuccess) return (int)e;
  }
  const int rc = riab::launch_agent_pub(a, r.side_s, state_published);
  if (rc) return rc;
  r.t_traj_launched = host_us();
  // MIRROR, the trajectory kernel is in flight (started_total: before any gate reads it; progress_end: only now):
  h->last_launches = r.d.open ? 2 : 1;
  h->started_total += r.n_traj;
  h->prev_ctrl = q->ctrl;
  h->prev_T = q->T;
  h->prev_walls = q->env->n_walls;
  h->prev_lead_row_bytes = 0;
  h->progress_end = (uint32_t)q->step0 + (uint32_t)q->T;
  h->progress_valid = true;
  return RIAB_OK;
}

// ---- forced positions: no recurrence, nothing to overlap: one stream, kernel after kernel --------------------------
// (last_launches stays 0 after such a call: riab_simulate_logic.h, planned_launches)
int issue_serial(SimRun& r, riab::AgentArgs& a) {
  const int rc = riab::launch_agent_forced(a, r.main_s);
  if (rc) return rc;
  r.h->last_form = r.d.form;
  int fail = RIAB_OK;
  for (int32_t t0 = 0; t0 < r.q->T && !fail; t0 += riab::SIM_SERIAL_PIECE) {
    const int32_t tc = r.q->T - t0 < riab::SIM_SERIAL_PIECE ? r.q->T - t0 : riab::SIM_SERIAL_PIECE;
    for (int i = 0; i < r.q->n_pops && !fail; ++i)
      fail = launch_pop_rows(r.q, i, t0, tc, r.main_s);
  }
  return fail ? RIAB_EPARTIAL : RIAB_OK;
}

// ---- a lead: [started gate,] the row-following kernel over the head, the lead's tail pieces, the other populations -----
int issue_lead(SimRun& r) {
  RiabStreamer* h = r.h;
  const RiabSimulate* q = r.q;
  const riab::SimDecision& d = r.d;
  const int32_t T = q->T;
  const bool timed_lead = d.timing && q->timed_pop == d.lead;
  int fail = RIAB_OK;
  // (the started gate is one sleeping wave; it may have to sit out whatever runs in front of the trajectory kernel)
  if (d.gate) {
    fail = riab::launch_stream_gate(q->ctrl, h->started_total, 0, 0, r.gate_limit(1u << 24), true, 0u, r.main_s);
    ++h->last_launches;
  }
  int n_timed = 0;
  if (timed_lead && !d.pure) (void)hipEventRecord(h->pairs[0], r.main_s);
  if (!fail) {
    fail = r.rate_stream(false, d.reserve);
    ++h->last_launches;
    r.note_first_rate_launch();
    if (d.head == T) h->prev_lead_row_bytes = d.lead_row_bytes;
  }
  for (int32_t t0 = d.head; t0 < T && !fail; t0 += riab::SIM_TAIL_PIECE) {
    const int32_t tc = T - t0 < riab::SIM_TAIL_PIECE ? T - t0 : riab::SIM_TAIL_PIECE;
    fail = riab::launch_stream_gate(q->ctrl, h->started_total, r.n_traj, (uint32_t)q->step0 + (uint32_t)(t0 + tc),
                                    r.gate_limit(1u << 22), false, 0u, r.main_s);
    if (!fail) fail = launch_pop_rows(q, d.lead, t0, tc, r.main_s);
    h->last_launches += 2;
  }
  if (timed_lead && !d.pure) {
    (void)hipEventRecord(h->pairs[1], r.main_s);
    n_timed = 1;
  }
  // (every workgroup of the row-following kernel has waited for its row, the last gate of a tail for row T: when the
  // lead's last kernel ends, all T rows are in memory, and the kernel boundary makes them visible to ordinary loads)
  // (last_launches does not count the launches of these other populations: planned_launches)
  for (int i = 0; i < q->n_pops && !fail; ++i) {
    if (i == d.lead) continue;
    for (int32_t t0 = 0; t0 < T && !fail; t0 += riab::SIM_REST_PIECE) {
      const int32_t tc = T - t0 < riab::SIM_REST_PIECE ? T - t0 : riab::SIM_REST_PIECE;
      const bool timed = d.timing && i == q->timed_pop;
      if (timed) (void)hipEventRecord(h->pairs[2 * n_timed], r.main_s);
      fail = launch_pop_rows(q, i, t0, tc, r.main_s);
      if (timed) {
        (void)hipEventRecord(h->pairs[2 * n_timed + 1], r.main_s);
        ++n_timed;
      }
    }
  }
  if (!fail && d.timing) {  // MIRROR, what riab_streamer_last_rate_ms reads:
    if (d.pure) {
      h->timed = d.events ? 1 : 2;
      h->stamp_ctrl = q->ctrl;
    } else {
      h->n_pairs = n_timed;
      h->timed = n_timed > 0 ? 1 : 0;
    }
  }
  return fail;
}

// ---- no lead: per chunk a progress gate, then every population's kernel over the chunk ------------------------------------
// (the first progress gate also waits until every trajectory workgroup of this launch is resident — it may have to
// sit out what is queued in front of the trajectory kernel — so there is no separate started gate)
int issue_chunks(SimRun& r) {
  RiabStreamer* h = r.h;
  const RiabSimulate* q = r.q;
  const riab::SimDecision& d = r.d;
  int fail = RIAB_OK;
  int32_t t0 = 0;
  for (size_t k = 0; k < d.sched.size() && !fail; ++k) {
    const int32_t tc = d.sched[k];
    // ~0.5 us per poll: seconds before a gate gives up (a healthy wait is one chunk of trajectory, < 1 ms)
    fail = riab::launch_stream_gate(q->ctrl, h->started_total, r.n_traj, (uint32_t)q->step0 + (uint32_t)(t0 + tc),
                                    r.gate_limit(k == 0 ? 1u << 24 : 1u << 22), false,
                                    (k == 0 && d.serial_rows) ? (uint32_t)q->step0 + (uint32_t)q->T : 0u, r.main_s);
    r.note_first_rate_launch();
    h->last_launches += 1 + q->n_pops;  // (counted before they are launched, also when the gate has just failed)
    for (int i = 0; i < q->n_pops && !fail; ++i) {
      if (d.timing && i == q->timed_pop) (void)hipEventRecord(h->pairs[2 * k], r.main_s);
      fail = launch_pop_rows(q, i, t0, tc, r.main_s);
      if (d.timing && i == q->timed_pop) (void)hipEventRecord(h->pairs[2 * k + 1], r.main_s);
    }
    t0 += tc;
  }
  if (!fail && d.timing) {  // MIRROR, what riab_streamer_last_rate_ms reads:
    h->n_pairs = (int)d.sched.size();
    h->timed = 1;
  }
  return fail;
}
}  // namespace

extern "C" int riab_simulate(RiabStreamer* h, const RiabSimulate* q, riab_stream_t stream) {
  riab::AgentArgs a;
  int rc = validate(h, q, a);
  if (rc) return rc;
  SimRun r = {h, q, {}, (hipStream_t)stream, nullptr, (uint32_t)((q->B + 63) / 64), 0.0, false};
  riab::SimDecision& d = r.d;
  // facts.  (The capture check comes first: a capturing stream must not be queried by anything below.)
  hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(r.main_s, &cap_status) == hipSuccess && cap_status != hipStreamCaptureStatusNone;
  std::vector<riab::SimPop> pops;
  riab::SimFacts f = gather_facts(h, q, r.main_s, capturing, pops);
  // decide, first step: the mode, the form
  riab::decide_mode(f, d);
  if (d.rc) return d.rc;
  // MIRROR, a call begins:
  h->timed = 0;
  h->n_pairs = 0;
  h->last_strict = d.strict ? 1 : 0;
  h->last_form = RIAB_FORM_NONE;
  h->last_launches = 0;
  riab::choose_lead(f, d);
  if (riab::calibration_due(f, d) && hipStreamQuery(r.main_s) == hipSuccess) {
    calibrate_from_stamps(h);
    f.calibrated = h->calibrated, f.step_ns_meas = h->step_ns_meas, f.lead_mbps_meas = h->lead_mbps_meas;
  }
  riab::decide_form(f, d);
  if (q->n_pops == 0) {  // an agent without populations: the trajectory alone, on the caller's stream
    h->last_launches = 1;
    return riab::launch_agent_plain(a, r.main_s);
  }
  if (q->forced_pos) return issue_serial(r, a);
  h->last_form = d.form;
  if (d.lead >= 0) {  // (dry runs: the row-following kernel's own argument checks; whether it offers its reserving shape)
    rc = r.rate_stream(true, false);
    if (rc) return rc;
    if (d.pure && h->gate_mode == RIAB_GATE_RESERVED) f.reservable = r.rate_stream(true, true) == RIAB_OK;
  }
  // provision the timing events (a strict call creates nothing: decide_form has turned its timing off instead)
  if (!ensure_pairs(h, d.pairs_needed, !d.strict)) return RIAB_EINVAL;
  // decide, second step: residency, once the caller's stream has been asked and the second stream is known
  f.idle = !d.strict && hipStreamQuery(r.main_s) == hipSuccess;
  if (!second_stream(h, r.main_s, d.strict, f.idle, &r.side_s)) return RIAB_EINVAL;
  f.side_differs = r.side_s != r.main_s;
  riab::decide_residency(f, d);
  bool state_published = false;
  rc = launch_trajectory(r, a, capturing, &state_published);
  if (rc) return rc;
  // From here on the state has advanced: a later failure still joins the two streams and is reported as RIAB_EPARTIAL
  // (the trajectory rows are complete, the rates of this call are not).
  const int fail = d.lead >= 0 ? issue_lead(r) : issue_chunks(r);
  hipError_t e = hipSuccess;
  if (riab::needs_join(d, state_published, fail != RIAB_OK)) {
    e = hipEventRecord(h->join, r.side_s);
    if (e == hipSuccess) e = hipStreamWaitEvent(r.main_s, h->join, 0);
  }
  if (fail) return RIAB_EPARTIAL;
  return e == hipSuccess ? RIAB_OK : (int)e;
}

extern "C" int riab_host_wait_spin(int32_t on) {
  // hipDeviceScheduleSpin: the host thread spins on the completion signal in hipDeviceSynchronize / hipStreamSynchronize
  // instead of blocking in the kernel driver after ~100 us of active waiting (the default): a region of a few kernels
  // ends 10-20 us sooner from the host's point of view, at the price of a busy core while it waits.
  const hipError_t e = hipSetDeviceFlags(on ? hipDeviceScheduleSpin : hipDeviceScheduleAuto);
  return e == hipSuccess ? RIAB_OK : (int)e;
}

extern "C" int64_t riab_abi_sizeof(int32_t which) {
  switch (which) {
    case 0: return (int64_t)sizeof(RiabEnv);
    case 1: return (int64_t)sizeof(RiabMotion);
    case 2: return (int64_t)sizeof(RiabRateIO);
    case 3: return (int64_t)sizeof(RiabPopulation);
    case 4: return (int64_t)sizeof(RiabTask);
    case 5: return (int64_t)sizeof(RiabFFInput);
    case 6: return (int64_t)RIAB_TS_ROWS;
    case 7: return (int64_t)sizeof(RiabSimulate);
    case 8: return (int64_t)sizeof(RiabWatch);
    case 9: return (int64_t)sizeof(RiabTDParams);
    case 10: return (int64_t)sizeof(RiabTDLayer);
    case 11: return (int64_t)sizeof(RiabMLPLayer);
    case 12: return (int64_t)sizeof(RiabMomentInput);
    default: return -1;
  }
}
