// Step plans: the per-step (closed-loop) path as ONE native call.
//
// `Agent.update(); N.update() for N in neurons` costs, from Python, one ctypes transition,
// struct filling and history bookkeeping per kernel — 30+ us per step at cfg 2 against ~9 us of
// GPU time.  A plan records the agent and its populations once (the same arguments the
// per-kernel entry points take); riab_plan_step then advances the row cursors, RNG counters and
// pointers in C++ and enqueues the motion kernel and every population's rate kernel for each
// requested step.  No allocation, no synchronisation: histories are chunks handed in by the
// caller, and the call reports RIAB_EFULL (before launching anything) when a chunk is exhausted.
#include <cstdlib>
#include <new>
#include <vector>

#include "riab_agent_kernel.h"
#include "riab_launch.h"

// A TD learner of the plan (riab_plan_set_learner): population `index` + what riab_td_learn_step takes beyond its rows
struct PlanLearner {
  int index;
  RiabTDParams p;
  float* trace[RIAB_FF_MAX_INPUTS];
  float *v_last, *dvdt, *td, *workspace;
  int64_t workspace_floats;
  int reward_kind;  // RIAB_REWARD_*
  const void* reward;
  int reward_f64;
  int64_t reward_ld_n, reward_ld_b;
  int reward_index;
};

struct RiabPlan {
  RiabEnv env;
  RiabMotion motion;
  double* state;
  int64_t B;
  int64_t agent_id0;
  uint64_t seed;
  uint64_t step;  // number of Agent.update() steps taken so far (the RNG counter)
  // Agent.t (riab_plan_set_clock): `clock` is the agent's time after `clock_step` updates; brought up to `step` by one
  // `clock += motion.dt` per step taken since (plan_clock), the operation the per-step loop performs on Agent.t
  double clock;
  uint64_t clock_step;
  const double* drift;
  // imported / forced trajectory (riab_plan_set_forced): positions of the coming steps, [rows][2][B]; null = motion model
  const double* forced;
  int64_t forced_rows, forced_fill;
  float* hist_base;     // [cap][8][B]
  int64_t hist_cap, hist_fill;
  float* row_scratch;   // [8][B] used when no history chunk is attached
  int32_t* diag;
  std::vector<RiabPopulation> pops;
  std::vector<int64_t> pop_fill;
  std::vector<PlanLearner> learners;  // in the order of their populations
  // attached task (riab_plan_set_task) whose lanes may be the agents of one world (riab_plan_set_task_world): the record
  // its launchers take.  tk.t_env and tk.counter are cursors like `step`; hist_x/y and gv_x/y are set per step (task_run)
  bool has_task;
  riab::TaskRun tk;
  double dt_env;
  bool action_ready;  // the drift buffer holds the scripted action of the coming step
  // the one-launch step (riab_plan_set_fused)
  uint32_t* sync_words;
  uint32_t epoch;        // tag of the last one-launch step on sync_words
  bool walls_ready;      // the wall table behind sync_words has been prepared (the plan's first one-launch step does it)
  int n_cus;             // compute units the plan's launches can occupy (riab_plan_set_compute_units)
  int fused_n;           // populations whose update() rides in the agent step's launch; -2: not worked out yet
  int fused[RIAB_STEP1_MAX_POPS];  // ... their indices, in list order
  bool fused_whole;      // ... worked out for whole-plan steps (riab_plan_step) / for the split entry points
  int64_t fused_steps, launches;
  // split entry points: riab_plan_step_agent wrote the rows of step `pre_step` of the populations flagged in
  // `pre_pending` ahead; a row nobody claimed (riab_plan_step_population) is a miss of its population
  std::vector<uint32_t> xch_arrivals;  // per population: arrivals its ray-exchange launches have asked of bvc_xch_count so far
  std::vector<char> pre_pending;  // per population
  uint64_t pre_step;
  std::vector<int> pre_misses;    // per population, in a row
};

static int fused_agent_step(RiabPlan* p, float* row, hipStream_t s, bool need_free_row, uint32_t* mask, bool query);

static double plan_clock(RiabPlan* p) {
  for (; p->clock_step < p->step; ++p->clock_step) p->clock += p->motion.dt;
  return p->clock;
}

// the tag of the next one-launch step on sync_words (never 0: that is a zeroed word); a query launches nothing and takes none
static uint32_t next_epoch(RiabPlan* p, bool query) {
  if (query) return 1u;
  p->epoch += 1u;
  if (p->epoch == 0u) p->epoch = 1u;
  return p->epoch;
}

// the compute units the plan's launches count on when nobody said (riab_plan_set_compute_units): the device's own count
static void default_compute_units(RiabPlan* p) {
  if (p->n_cus > 0) return;
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 1;
  p->n_cus = n;
}

// the plan's task record with the values of the step that writes `row` (null: the launch patches the row it stores itself)
static const riab::TaskRun& task_run(RiabPlan* p, float* row) {
  riab::TaskRun& t = p->tk;
  double* const act = t.gv_scale > 0.0 ? const_cast<double*>(p->drift) : nullptr;
  t.gv_x = act;
  t.gv_y = act ? act + p->B : nullptr;
  t.hist_x = row ? row + (int64_t)RIAB_H_POS_X * p->B : nullptr;
  t.hist_y = row ? row + (int64_t)RIAB_H_POS_Y * p->B : nullptr;
  return t;
}

// this step's rows of the plan's fused populations (split: those whose chunk has a free row); returns how many
static int fused_refs(const RiabPlan* p, riab::Step1PopRef* refs, uint32_t* mask, bool need_free_row) {
  int n = 0;
  *mask = 0u;
  for (int k = 0; k < p->fused_n; ++k) {
    const int i = p->fused[k];
    const RiabPopulation& q = p->pops[i];
    if (need_free_row && q.capacity_rows > 0 && p->pop_fill[i] >= q.capacity_rows) continue;
    const int64_t r = q.capacity_rows > 0 ? p->pop_fill[i] : 0;
    const int64_t row_elems = (int64_t)q.n * p->B;
    refs[n].pop = &q;
    refs[n].rates_row = q.rates_base + r * row_elems;
    refs[n].spikes_row = q.spikes_base ? q.spikes_base + r * row_elems : nullptr;
    *mask |= 1u << k;
    ++n;
  }
  return n;
}

// One closed-loop step of a plan with a task as ONE kernel: Agent.update(), the rest of TaskEnvironment.step (+ the caller's
// `if terminal: reset()`, + the next scripted action) and the fused populations' update().  The caller has advanced the
// plan's cursors: this reads p->step - 1.  `query`: nothing is launched; RIAB_OK when there is a kernel for this plan's step.
static int fused_task_step(RiabPlan* p, float* row, hipStream_t s, bool query) {
  riab::AgentArgs ma;
  const uint64_t step_before = query ? p->step : p->step - 1;
  int rc = riab::fill_agent_args(ma, &p->env, &p->motion, p->state, p->B, p->agent_id0, p->drift, nullptr, nullptr, nullptr, p->seed,
                                 step_before, 1, row, p->diag);
  if (rc) return rc;
  const riab::TaskRun& t = task_run(p, nullptr);
  if (t.gv_scale > 0.0 && (!t.gv_x || !p->motion.has_drift)) return RIAB_EINVAL;
  riab::Step1PopRef refs[RIAB_STEP1_MAX_POPS];
  uint32_t mask;
  const int n = fused_refs(p, refs, &mask, false);
  const uint32_t epoch = next_epoch(p, query);
  rc = riab::launch_step1_task(ma, &p->env, refs, n, p->seed, step_before + 1, p->sync_words, epoch, &p->walls_ready, p->n_cus, t,
                               s, query);
  if (rc == RIAB_OK && !query) {
    p->fused_steps += 1;
    p->launches += 1;
  }
  return rc;
}

// The populations whose update() rides in the agent step's launch: every store-bound one without additive noise the
// one-launch step has a functor for (riab_step1.hip: step1_supported), up to RIAB_STEP1_MAX_POPS of them — the ones
// that write most bytes per row —, in list order.  Returns how many (0: the step is launched kernel by kernel).
// `whole_step`: for riab_plan_step; otherwise for the split entry points, where a population that keeps no history
// (its one row is what `firingrate` shows until ITS update() call) and one the caller's loop does not update after
// every agent step are left out.  (a plan with a task: whole-plan steps only, motion + task fused (RIAB_OPT_FUSED_TASK))
static int plan_fused(RiabPlan* p, bool whole_step = false) {
  if (!p->sync_words || riab::g_options[RIAB_OPT_FUSED_STEP] == 0 || p->forced) return 0;
  if (p->has_task && (!whole_step || riab::g_options[RIAB_OPT_FUSED_TASK] == 0)) return 0;
  if (p->has_task && !p->learners.empty()) return 0;  // (the TASK modes reset inside the kernel: a learner's step resets last)
  if (p->fused_n == -2 || p->fused_whole != whole_step) {
    p->fused_whole = whole_step;
    p->pre_misses.resize(p->pops.size(), 0);
    p->pre_pending.resize(p->pops.size(), 0);
    default_compute_units(p);
    int cand[RIAB_STEP1_MAX_POPS];
    int64_t bytes[RIAB_STEP1_MAX_POPS];
    int n = 0;
    for (size_t i = 0; i < p->pops.size(); ++i) {
      const RiabPopulation& q = p->pops[i];
      if (riab::step1_supported(&p->env, &q, p->B) != RIAB_OK) continue;
      if (!whole_step && (q.capacity_rows == 0 || p->pre_misses[i] >= 2)) continue;
      const int64_t b = (int64_t)q.n * (q.spikes_base ? 5 : 4);
      if (n < RIAB_STEP1_MAX_POPS) {
        cand[n] = (int)i;
        bytes[n] = b;
        ++n;
        continue;
      }
      int least = 0;  // (more candidates than slots: the smallest gives way; the list order of the others is kept)
      for (int k = 1; k < n; ++k)
        if (bytes[k] < bytes[least]) least = k;
      if (bytes[least] >= b) continue;
      for (int k = least; k + 1 < n; ++k) {
        cand[k] = cand[k + 1];
        bytes[k] = bytes[k + 1];
      }
      cand[n - 1] = (int)i;
      bytes[n - 1] = b;
    }
    p->fused_n = n;
    for (int k = 0; k < n; ++k) p->fused[k] = cand[k];
    uint32_t mask;  // (is there a kernel and a grid for it on this device?)
    if (n > 0 && (p->has_task ? fused_task_step(p, p->row_scratch, nullptr, true)
                              : fused_agent_step(p, p->row_scratch, nullptr, false, &mask, true)) != RIAB_OK)
      p->fused_n = 0;
  }
  return p->fused_n;
}
static bool is_fused(const RiabPlan* p, int index) {
  for (int k = 0; k < p->fused_n; ++k)
    if (p->fused[k] == index) return true;
  return false;
}

// Agent.update() + the fused populations' update() of the same step as one kernel; cursors are the caller's business.
// `mask`: which of the fused populations took part (split entry points: the ones with a free row).
// (`query`: nothing is launched; RIAB_OK when there is a kernel and a grid for this plan's step)
static int fused_agent_step(RiabPlan* p, float* row, hipStream_t s, bool need_free_row, uint32_t* mask, bool query) {
  riab::Step1PopRef refs[RIAB_STEP1_MAX_POPS];
  const int n = fused_refs(p, refs, mask, need_free_row);
  if (n == 0) return RIAB_EUNSUPPORTED;
  riab::AgentArgs ma;
  int rc = riab::fill_agent_args(ma, &p->env, &p->motion, p->state, p->B, p->agent_id0, p->drift, nullptr, nullptr, nullptr,
                                 p->seed, p->step, 1, row, p->diag);
  if (rc) return rc;
  const uint32_t epoch = next_epoch(p, query);
  rc = riab::launch_step1(ma, &p->env, refs, n, p->seed, p->step + 1, p->sync_words, epoch, &p->walls_ready, p->n_cus, s, query);
  if (rc == RIAB_OK && !query) {
    p->fused_steps += 1;
    p->launches += 1;
  }
  return rc;
}

extern "C" RiabPlan* riab_plan_create(const RiabEnv* env, const RiabMotion* motion, double* state, int64_t B,
                                      int64_t agent_id0, uint64_t seed, uint64_t step, float* row_scratch,
                                      int32_t* diag) {
  if (!env || !motion || !state || B <= 0 || !row_scratch) return nullptr;
  RiabPlan* p = new (std::nothrow) RiabPlan();
  if (!p) return nullptr;
  p->env = *env;
  p->motion = *motion;
  p->state = state;
  p->B = B;
  p->agent_id0 = agent_id0;
  p->seed = seed;
  p->step = step;
  p->clock = 0.0;
  p->clock_step = step;
  p->drift = nullptr;
  p->forced = nullptr;
  p->forced_rows = p->forced_fill = 0;
  p->hist_base = nullptr;
  p->hist_cap = p->hist_fill = 0;
  p->row_scratch = row_scratch;
  p->diag = diag;
  p->has_task = false;
  p->tk = riab::TaskRun();
  p->action_ready = false;
  p->sync_words = nullptr;
  p->epoch = 0u;
  p->walls_ready = false;
  p->n_cus = 0;
  p->fused_n = -2;
  p->fused_whole = false;
  p->fused_steps = p->launches = 0;
  p->pre_step = 0;
  return p;
}

extern "C" int riab_plan_set_fused(RiabPlan* p, uint32_t* sync_words, int64_t n_words) {
  if (!p || n_words < 0) return RIAB_EINVAL;
  if (sync_words && n_words < (int64_t)RIAB_STEP1_SYNC_WORDS(p->B)) return RIAB_EINVAL;
  if (((uintptr_t)sync_words) & 7) return RIAB_EALIGN;  // (the mail's 8-byte entries, the prepared walls' float64)
  p->sync_words = sync_words;
  p->epoch = 0u;
  p->walls_ready = false;
  p->fused_n = -2;
  p->pre_pending.assign(p->pops.size(), 0);
  p->pre_misses.assign(p->pops.size(), 0);
  return RIAB_OK;
}

extern "C" int riab_plan_set_compute_units(RiabPlan* p, int32_t n_cus) {
  if (!p || n_cus < 0) return RIAB_EINVAL;
  p->n_cus = n_cus;  // (0: the device's own count, asked at the next one-launch step)
  p->fused_n = -2;
  return RIAB_OK;
}

extern "C" int64_t riab_plan_info(const RiabPlan* p, int32_t which) {
  if (!p) return 0;
  switch (which) {
    case 0: return p->fused_steps;
    case 1: return p->fused_n <= 0 ? -1 : p->fused[0];
    case 2: return p->launches;
    case 3: return p->sync_words ? 1 : 0;
    case 4: return p->fused_n < 0 ? 0 : p->fused_n;
    case 5: return p->n_cus;
    default:
      if (which >= 8 && which < 8 + RIAB_STEP1_MAX_POPS) return which - 8 < p->fused_n ? p->fused[which - 8] : -1;
      return 0;
  }
}

extern "C" void riab_plan_destroy(RiabPlan* p) { delete p; }

extern "C" int riab_plan_set_motion(RiabPlan* p, const RiabMotion* motion, const double* drift) {
  if (!p || !motion) return RIAB_EINVAL;
  if (motion->has_drift && !drift) return RIAB_EINVAL;
  plan_clock(p);  // (the steps taken so far advanced the clock by the dt they were taken at)
  if (motion->wall_repel_distance_kw != p->motion.wall_repel_distance_kw) p->walls_ready = false;  // (the box fast path's verdict depends on it)
  p->motion = *motion;
  p->drift = drift;
  p->action_ready = false;
  return RIAB_OK;
}

// Agent._update_position_along_imported_trajectory / forced_next_position (Agent.py:229-266) for the coming
// `n_rows` steps: every agent step of the plan then MOVES the agents to the next row of `forced` ([n_rows][2][B],
// float64, device) instead of running the motion model; RIAB_EFULL once the rows are used up (set the next ones).
extern "C" int riab_plan_set_forced(RiabPlan* p, const double* forced, int64_t n_rows) {
  if (!p || n_rows < 0 || (forced && n_rows == 0) || p->has_task) return RIAB_EINVAL;
  p->forced = forced;
  p->forced_rows = forced ? n_rows : 0;
  p->forced_fill = 0;
  return RIAB_OK;
}

extern "C" int riab_plan_set_agent_history(RiabPlan* p, float* hist_base, int64_t capacity_rows) {
  if (!p || capacity_rows < 0 || (capacity_rows > 0 && !hist_base)) return RIAB_EINVAL;
  p->hist_base = hist_base;
  p->hist_cap = capacity_rows;
  p->hist_fill = 0;
  return RIAB_OK;
}

// What a population must satisfy wherever it is launched from (a step plan, riab_simulate): no more objects than the
// vector-cell kernel stages, and every input of a feed-forward layer among the `n_before` populations ahead of it.
int riab::check_population(const RiabPopulation& q, int n_before) {
  if (q.kind == RIAB_POP_OVC) {
    const int limit = ovc_object_limit();
    if (limit >= 0 && q.n_objects > limit) return RIAB_ETOOBIG;
  }
  if (q.kind == RIAB_POP_FF) {
    if (q.n_inputs <= 0 || q.n_inputs > RIAB_FF_MAX_INPUTS) return RIAB_EINVAL;
    for (int l = 0; l < q.n_inputs; ++l)
      if (q.input_index[l] < 0 || q.input_index[l] >= n_before) return RIAB_EINVAL;
  }
  return RIAB_OK;
}

extern "C" int riab_plan_add(RiabPlan* p, const RiabPopulation* pop) {
  if (!p || !pop || pop->n <= 0 || !riab::population_kind_known(pop->kind)) return RIAB_EINVAL;
  // (a plan that could not take its first step is refused when it is recorded; feed-forward only: an input must already
  // be in the plan)
  const int rc = riab::check_population(*pop, (int)p->pops.size());
  if (rc) return rc;
  if (pop->kind == RIAB_POP_THETA_PLACE && (!pop->table || !(pop->theta_freq > 0.0) || !(pop->kappa >= 0.0))) return RIAB_EINVAL;
  if (pop->kind == RIAB_POP_PLANE_WAVE && !pop->table) return RIAB_EINVAL;
  if (pop->kind == RIAB_POP_FF) {
    if (!pop->bias) return RIAB_EINVAL;
    for (int l = 0; l < pop->n_inputs; ++l)
      if (!pop->input_wt[l]) return RIAB_EINVAL;
  }
  p->pops.push_back(*pop);
  p->pop_fill.push_back(0);
  p->pre_misses.push_back(0);
  p->pre_pending.push_back(0);
  p->fused_n = -2;
  return (int)p->pops.size() - 1;
}

// Neurons.update reads Agent.dt (Neurons.py:153-168): a step at a new dt takes the noisy populations' OU constants with it
extern "C" int riab_plan_set_noise(RiabPlan* p, int32_t index, float theta_dt, float sigma_dt) {
  if (!p || index < 0 || index >= (int)p->pops.size() || !p->pops[index].noise_state) return RIAB_EINVAL;
  p->pops[index].noise_theta_dt = theta_dt;
  p->pops[index].noise_sigma_dt = sigma_dt;
  return RIAB_OK;
}

extern "C" int riab_plan_set_population_history(RiabPlan* p, int32_t index, float* rates_base, uint8_t* spikes_base,
                                                int64_t capacity_rows) {
  if (!p || index < 0 || index >= (int)p->pops.size() || capacity_rows < 0) return RIAB_EINVAL;
  if (!rates_base) return RIAB_EINVAL;  // capacity 0 = a single-row scratch that is overwritten every step
  RiabPopulation& q = p->pops[index];
  q.rates_base = rates_base;
  q.spikes_base = spikes_base;
  q.capacity_rows = capacity_rows;
  p->pop_fill[index] = 0;
  p->pre_pending[index] = 0;  // (a row written ahead was in the old chunk)
  p->fused_n = -2;            // (spikes or not changes the bytes a row takes)
  return RIAB_OK;
}

extern "C" int riab_plan_set_task(RiabPlan* p, const RiabTask* task, double* task_state, int64_t task_B, double t_env,
                                  double dt_env, double* reward_out, uint8_t* terminal_out, int32_t* task_diag,
                                  int32_t auto_reset, int32_t n_select, int32_t ordered, uint64_t task_seed,
                                  uint64_t reset_counter, int32_t teleport, double* ep_log, int64_t ep_log_cap,
                                  int32_t* ep_count, double scripted_speed) {
  if (!p) return RIAB_EINVAL;
  p->fused_n = -2;
  p->pre_pending.assign(p->pops.size(), 0);
  p->tk.world = nullptr;
  if (!task) {
    p->has_task = false;
    return RIAB_OK;
  }
  if (!task_state || task_B <= 0 || task_B > p->B || !reward_out || !terminal_out || !task_diag) return RIAB_EINVAL;
  if (n_select < 0 || n_select > RIAB_TASK_MAX_GOALS - 1) return RIAB_ETOOBIG;
  if (ep_log && (!ep_count || ep_log_cap <= 0)) return RIAB_EINVAL;
  p->has_task = true;
  riab::TaskRun& t = p->tk;
  t = riab::TaskRun();
  t.env = &p->env;
  t.task = *task;
  t.task_state = task_state;
  t.task_B = task_B;
  t.pos_x = p->state + (int64_t)RIAB_S_POS_X * p->B;
  t.pos_y = p->state + (int64_t)RIAB_S_POS_Y * p->B;
  t.reward_out = reward_out;
  t.terminal_out = terminal_out;
  t.diag = task_diag;
  t.auto_reset = auto_reset;
  t.n_select = n_select;
  t.ordered = ordered;
  t.teleport = teleport;
  t.agent_id0 = p->agent_id0;
  t.seed = task_seed;
  t.ep_log = ep_log;
  t.ep_log_cap = ep_log_cap;
  t.ep_count = ep_count;
  t.gv_scale = scripted_speed;
  t.t_env = t_env;
  t.counter = reset_counter;
  p->dt_env = dt_env;
  p->action_ready = false;
  return RIAB_OK;
}

extern "C" int riab_plan_set_task_world(RiabPlan* p, double* world, uint64_t* met_scratch, int32_t* cand_scratch, int32_t* ctl) {
  if (!p || !p->has_task) return RIAB_EINVAL;
  if (world && (!met_scratch || !cand_scratch || !ctl)) return RIAB_EINVAL;
  p->tk.world = world;
  p->tk.world_met = met_scratch;
  p->tk.world_cand = cand_scratch;
  p->tk.world_ctl = ctl;
  p->fused_n = -2;
  return RIAB_OK;
}

extern "C" int riab_plan_set_learner(RiabPlan* p, int32_t index, const RiabTDParams* prm, float* const* traces, float* v_last,
                                     float* dvdt, float* td, float* workspace, int64_t workspace_floats, int32_t reward_kind,
                                     const void* reward, int32_t reward_f64, int64_t reward_ld_n, int64_t reward_ld_b,
                                     int32_t reward_index) {
  if (!p || !prm || !traces || index < 0 || index >= (int)p->pops.size()) return RIAB_EINVAL;
  const RiabPopulation& q = p->pops[index];
  if (q.kind != RIAB_POP_FF || !q.rates_prime) return RIAB_EINVAL;
  if (prm->n != q.n || prm->Bp != p->B) return RIAB_EINVAL;
  if (!v_last || !dvdt || !td || !workspace) return RIAB_EINVAL;
  if (reward_kind < RIAB_REWARD_NONE || reward_kind > RIAB_REWARD_POPULATION) return RIAB_EINVAL;
  PlanLearner L = {};
  L.index = index;
  L.p = *prm;
  RiabTDLayer layers[RIAB_FF_MAX_INPUTS];
  for (int l = 0; l < q.n_inputs; ++l) {  // (the rates are this step's rows, resolved per step: the check gets the trace's)
    L.trace[l] = traces[l];
    layers[l].rates = traces[l];
    layers[l].trace = traces[l];
    layers[l].wt = const_cast<float*>(q.input_wt[l]);
    layers[l].n_in = p->pops[q.input_index[l]].n;
  }
  const int rc = riab::td_check(prm, layers, q.n_inputs);
  if (rc) return rc;
  if ((((uintptr_t)v_last | (uintptr_t)dvdt | (uintptr_t)td | (uintptr_t)workspace | (uintptr_t)q.rates_prime) & 15)) return RIAB_EALIGN;
  if (workspace_floats < riab_td_workspace(prm, layers, q.n_inputs)) return RIAB_EINVAL;
  if (reward_kind == RIAB_REWARD_POINTER) {
    if (!reward || reward_ld_n < 0 || reward_ld_b < 0) return RIAB_EINVAL;
    if (((uintptr_t)reward & (reward_f64 ? 7 : 3))) return RIAB_EALIGN;
  }
  if (reward_kind == RIAB_REWARD_POPULATION && (reward_index < 0 || reward_index >= index || p->pops[reward_index].n != q.n))
    return RIAB_EINVAL;
  L.v_last = v_last;
  L.dvdt = dvdt;
  L.td = td;
  L.workspace = workspace;
  L.workspace_floats = workspace_floats;
  L.reward_kind = reward_kind;
  L.reward = reward;
  L.reward_f64 = reward_f64;
  L.reward_ld_n = reward_ld_n;
  L.reward_ld_b = reward_ld_b;
  L.reward_index = reward_index;
  size_t k = 0;  // (kept in the order of the populations; the same index again: the record is replaced)
  while (k < p->learners.size() && p->learners[k].index < index) ++k;
  if (k < p->learners.size() && p->learners[k].index == index) p->learners[k] = L;
  else p->learners.insert(p->learners.begin() + k, L);
  p->fused_n = -2;
  return RIAB_OK;
}

extern "C" double riab_plan_task_clock(const RiabPlan* p) { return p && p->has_task ? p->tk.t_env : 0.0; }

extern "C" int riab_plan_set_clock(RiabPlan* p, double t) {
  if (!p || !(t == t)) return RIAB_EINVAL;
  p->clock = t;
  p->clock_step = p->step;
  return RIAB_OK;
}

extern "C" double riab_plan_clock(const RiabPlan* p) { return p ? plan_clock(const_cast<RiabPlan*>(p)) : 0.0; }

extern "C" int64_t riab_plan_rows_free(const RiabPlan* p) {
  if (!p) return 0;
  int64_t free_rows = p->hist_base ? p->hist_cap - p->hist_fill : INT64_MAX;
  for (size_t i = 0; i < p->pops.size(); ++i) {
    if (p->pops[i].capacity_rows == 0) continue;  // single-row scratch (no history kept)
    const int64_t f = p->pops[i].capacity_rows - p->pop_fill[i];
    free_rows = f < free_rows ? f : free_rows;
  }
  return free_rows;
}

extern "C" uint64_t riab_plan_step_index(const RiabPlan* p) { return p ? p->step : 0; }

// Neurons.update() of one population on T successive history rows: the population's kernel, then — for a population with
// additive OU noise — the noise pass and the spikes drawn on the final rates.  The one launcher of a step plan's one-row
// launches and of riab_simulate's chunks; where the two differ, the record says so:
//   io.step0      plan: its step cursor, already advanced | simulate: step0 + 1 + t0
//   BVC           plan: the ray exchange (r.xch_arrivals, r.n_cus resolved by the caller) | simulate: no exchange (null, 0)
//   FeedForward   plan: T = 1, input j read at r.cursors[j] - 1 (row 0 without history), rates_prime written |
//                 simulate: T = tc, inputs read at rate_row = t0, rates_prime not written
//   velocity and phase-precessing cells read r.state and r.clock: a plan's; riab_simulate refuses them with
//                 RIAB_EUNSUPPORTED before anything is launched (check_populations)
//   `launches`    plan: += 1, + 1 for a layer's spike pass, + 1 or 2 for noise (with spikes) | simulate: null
int riab::launch_population_rows(const PopRows& r, hipStream_t s, int64_t* launches) {
  const RiabEnv* env = r.env;
  const RiabPopulation& q = r.pops[r.index];
  const int64_t B = r.B;
  RiabRateIO io = q.io;
  hist_rows_io(&io, r.hist, B, r.hist_ld);
  io.T = r.T;
  io.rates = q.rates_base + r.rate_row * q.n * B;
  io.spikes = q.spikes_base ? q.spikes_base + r.rate_row * q.n * B : nullptr;
  io.u_in = nullptr;
  io.dt = r.dt;
  io.seed = r.seed;
  io.step0 = r.step0;
  io.agent_id0 = r.agent_id0;
  const bool noisy = q.noise_state != nullptr;
  uint8_t* const spikes = io.spikes;
  if (noisy) io.spikes = nullptr;  // spikes are drawn on the final rate, after the noise has been added
  // (a kind without a case, a reader of the state without one: RIAB_EUNSUPPORTED, not reachable behind the callers' checks)
  int rc = RIAB_EUNSUPPORTED;
  switch (q.kind) {
    case RIAB_POP_PLACE: rc = riab_place_cells(env, &io, q.table, q.n, q.description, q.geometry, q.top_hat_width, s); break;
    case RIAB_POP_GRID: rc = riab_grid_cells(&io, q.table, q.n, q.description, q.f0, s); break;
    case RIAB_POP_HDC: rc = riab_head_direction_cells(&io, q.table, q.n, s); break;
    case RIAB_POP_PLANE_WAVE: rc = riab_plane_wave_neurons(&io, q.table, q.n, s); break;
    case RIAB_POP_VELOCITY:  // Agent.velocity: rows of the float64 state, not of the history record
      if (!r.state) break;
      rc = riab_velocity_cells(&io, q.table, q.n, q.one_sigma_speed, r.state + RIAB_S_VEL_X * B, r.state + RIAB_S_VEL_Y * B, s);
      break;
    case RIAB_POP_THETA_PLACE:  // Agent.velocity and Agent.t: the float64 state rows and the plan's clock
      if (!r.state) break;
      rc = riab_phase_precessing_place_cells(env, &io, q.table, q.n, q.description, q.geometry, q.top_hat_width, q.kappa,
                                             q.theta_freq * fmod(r.clock, 1.0 / q.theta_freq), r.state + RIAB_S_VEL_X * B,
                                             r.state + RIAB_S_VEL_Y * B, s);
      break;
    case RIAB_POP_SPEED:  // history["vel"]: the measured velocity of the steps just taken
      io.hd_x = r.hist + RIAB_H_VEL_X * B;
      io.hd_y = r.hist + RIAB_H_VEL_Y * B;
      rc = riab_speed_cell(&io, q.one_sigma_speed, s);
      break;
    case RIAB_POP_RANDOM_SPATIAL:
      rc = riab_random_spatial_neurons(env, &io, q.table, q.n_anchors, q.targets, q.n, q.geometry, s);
      break;
    case RIAB_POP_BVC: {
      const bool xch = r.xch_arrivals != nullptr;
      rc = launch_bvc(env, &io, q.test_dirs, q.ray_rden, q.K, q.table, q.vm_table, q.inv_norm, q.n, q.egocentric, nullptr,
                      q.cell_rows, q.windows, xch ? q.bvc_xch : nullptr, xch ? q.bvc_xch_count : nullptr, r.xch_arrivals,
                      xch ? r.n_cus : 0, s);
      break;
    }
    case RIAB_POP_OVC:
      rc = riab_object_vector_cells(env, &io, q.objects, q.object_types, q.n_objects, q.table, q.n, q.walls_occlude,
                                    q.egocentric, s);
      break;
    case RIAB_POP_FF: {
      RiabFFInput in[RIAB_FF_MAX_INPUTS];
      for (int l = 0; l < q.n_inputs; ++l) {
        const int j = q.input_index[l];
        const RiabPopulation& src = r.pops[j];  // (an earlier population: its rows of this step / chunk exist)
        const int64_t row_j = !r.cursors ? r.rate_row : (src.capacity_rows > 0 ? r.cursors[j] - 1 : 0);
        in[l].rates = src.rates_base + row_j * src.n * B;
        in[l].wt = q.input_wt[l];
        in[l].n_in = src.n;
      }
      rc = riab_feedforward(in, q.n_inputs, q.bias, q.n, r.T, B, q.activation, q.act_params, io.rates,
                            r.write_prime ? q.rates_prime : nullptr, s);
      if (rc == RIAB_OK && io.spikes) rc = riab_spikes(&io, q.n, s);
      break;
    }
  }
  if (rc) return rc;
  if (launches) *launches += (q.kind == RIAB_POP_FF && io.spikes) ? 2 : 1;
  if (noisy) {
    if (launches) *launches += spikes ? 2 : 1;
    rc = riab_neuron_noise(q.noise_state, io.rates, nullptr, q.n, B, r.T, q.noise_theta_dt, q.noise_sigma_dt, r.seed, r.step0,
                           q.io.pop_id, r.agent_id0, s);
    if (rc) return rc;
    if (spikes) {
      io.spikes = spikes;
      rc = riab_spikes(&io, q.n, s);
    }
  }
  return rc;
}

// Neurons.update() of population i on the history row `row`, after the p->step-th Agent.update() (the cursor was advanced)
static int launch_population(RiabPlan* p, size_t i, const float* row, hipStream_t s) {
  riab::PopRows r = {};
  r.env = &p->env;
  r.pops = p->pops.data();
  r.index = (int)i;
  r.hist = row;
  r.hist_ld = p->B;
  r.B = p->B;
  r.T = 1;
  r.rate_row = p->pop_fill[i];
  r.dt = (float)p->motion.dt;
  r.seed = p->seed;
  r.step0 = p->step;
  r.agent_id0 = p->agent_id0;
  r.state = p->state;
  if (p->pops[i].kind == RIAB_POP_THETA_PLACE) r.clock = plan_clock(p);
  if (p->pops[i].kind == RIAB_POP_BVC) {
    default_compute_units(p);
    if (p->xch_arrivals.size() < p->pops.size()) p->xch_arrivals.resize(p->pops.size(), 0u);
    r.xch_arrivals = &p->xch_arrivals[i];
    r.n_cus = p->n_cus;
  }
  r.cursors = p->pop_fill.data();  // (population j < i has been launched this step already: its cursor points past the row it wrote)
  r.write_prime = true;
  return riab::launch_population_rows(r, s, &p->launches);
}

// A row written ahead (riab_plan_step_agent) that its population did not claim is a miss of that population; two in a row
// leave it out of the one-launch step.
static void count_missed_rows(RiabPlan* p) {
  for (size_t i = 0; i < p->pre_pending.size(); ++i) {
    if (!p->pre_pending[i]) continue;
    p->pre_pending[i] = 0;
    if (++p->pre_misses[i] == 2) p->fused_n = -2;
  }
}

// One step taken: the RNG counter and the agent's history row; `task`: the task's clock too, and the counter of the
// resets the plan decides on the device.
static void advance_cursors(RiabPlan* p, bool task) {
  p->step += 1;
  if (p->hist_base) p->hist_fill += 1;
  if (task) {
    p->tk.t_env += p->dt_env;
    if (p->tk.auto_reset) p->tk.counter += 1;
  }
}

// The two halves of a plan step, for callers that keep the reference's call structure — `Ag.update()` here,
// `N.update()` there (demos/simple_example.ipynb cell 4) — and only want each call to cost one native transition:
// the same kernels, arguments and counters as riab_plan_step, so the same results bit for bit.  No task attached.
extern "C" int riab_plan_step_agent(RiabPlan* p, riab_stream_t stream) {
  if (!p || p->has_task) return RIAB_EINVAL;
  if (!p->learners.empty()) return RIAB_EUNSUPPORTED;  // (a learner's stage belongs to whole steps: riab_plan_step)
  if (p->hist_base && p->hist_fill >= p->hist_cap) return RIAB_EFULL;
  const double* forced = nullptr;
  if (p->forced) {
    if (p->forced_fill >= p->forced_rows) return RIAB_EFULL;
    forced = p->forced + p->forced_fill * 2 * p->B;
  }
  float* row = p->hist_base ? p->hist_base + p->hist_fill * (int64_t)RIAB_HIST_ROWS * p->B : p->row_scratch;
  // The one-launch step: the fused populations' rows of THIS step are written by the agent's launch, ahead of the
  // populations' own calls, which then only move their cursors (same inputs, same rows, same bits).  A row written ahead
  // that nobody claims (a loop that does not update that population after every agent step) is a miss; two in a row
  // leave the population out.
  count_missed_rows(p);
  if (plan_fused(p) > 0) {
    uint32_t mask = 0u;
    const int rc = fused_agent_step(p, row, (hipStream_t)stream, true, &mask, false);
    if (rc == RIAB_OK) {
      advance_cursors(p, false);
      for (int k = 0; k < p->fused_n; ++k)
        if (mask & (1u << k)) p->pre_pending[p->fused[k]] = 1;
      p->pre_step = p->step;
      return RIAB_OK;
    }
    if (rc != RIAB_EUNSUPPORTED) return rc;  // (no fused population has a free row: the plain agent step)
  }
  const int rc = riab_agent_step(&p->env, &p->motion, p->state, p->B, p->agent_id0, p->drift, nullptr, nullptr, forced, nullptr,
                                 p->seed, p->step, 1, row, p->diag, (hipStream_t)stream);
  if (rc) return rc;
  p->launches += 1;
  if (forced) p->forced_fill += 1;
  advance_cursors(p, false);
  return RIAB_OK;
}

// Something the fused populations read was edited after riab_plan_step_agent wrote their rows ahead (a TaskEnvironment
// reset teleported agents and patched the newest history row): the rows are not claimed — each population's own call
// launches its kernel on the edited row, which overwrites them.  Counted like a miss: a loop that discards every step
// (`env.reset(mask)` after every step) pays the fused work AND the populations' kernels, so two in a row switch the
// one-launch step off for them; one claimed row switches it on again.
extern "C" int riab_plan_discard_ahead(RiabPlan* p) {
  if (!p) return RIAB_EINVAL;
  count_missed_rows(p);
  return RIAB_OK;
}

// Neurons.update() of population `index` on the agent's newest history row
extern "C" int riab_plan_step_population(RiabPlan* p, int32_t index, riab_stream_t stream) {
  if (!p || p->has_task || index < 0 || index >= (int)p->pops.size()) return RIAB_EINVAL;
  if (!p->learners.empty()) return RIAB_EUNSUPPORTED;
  const size_t i = (size_t)index;
  if (p->pops[i].capacity_rows > 0 && p->pop_fill[i] >= p->pops[i].capacity_rows) return RIAB_EFULL;
  if (p->hist_base && p->hist_fill == 0) return RIAB_EINVAL;  // no agent row written into this chunk yet
  if (i < p->pre_pending.size() && p->pre_pending[i] && p->pre_step == p->step) {  // written by this step's riab_plan_step_agent
    p->pre_pending[i] = 0;
    p->pre_misses[i] = 0;
    if (p->pops[i].capacity_rows > 0) p->pop_fill[i] += 1;
    return RIAB_OK;
  }
  const float* row = p->hist_base ? p->hist_base + (p->hist_fill - 1) * (int64_t)RIAB_HIST_ROWS * p->B : p->row_scratch;
  const int rc = launch_population(p, i, row, (hipStream_t)stream);
  if (rc) return rc;
  if (i < p->pre_misses.size() && p->pre_misses[i] >= 2 && ++p->pre_misses[i] >= 2 + 64) {  // (left out: looked at again every 64 updates)
    p->pre_misses[i] = 0;
    p->fused_n = -2;
  }
  if (p->pops[i].capacity_rows > 0) p->pop_fill[i] += 1;
  return RIAB_OK;
}

// The scripted action of the plan's FIRST step (and of every step without auto-reset): later steps get theirs from the
// previous step's task / reset launch (action_ready).
static int first_action(RiabPlan* p, hipStream_t s) {
  const riab::TaskRun& t = p->tk;
  double* act = const_cast<double*>(p->drift);
  if (!act || !p->motion.has_drift) return RIAB_EINVAL;
  if (p->action_ready) return RIAB_OK;
  const int rc = t.world ? riab_task_world_goal_vector(&p->env, &t.task, t.task_state, t.world, t.pos_x, t.pos_y, t.task_B,
                                                       t.gv_scale, act, act + p->B, s)
                         : riab_task_goal_vector(&p->env, &t.task, t.task_state, t.pos_x, t.pos_y, t.task_B, t.gv_scale, act,
                                                 act + p->B, s);
  if (rc == RIAB_OK) p->launches += 1;
  return rc;
}

// Agent.update() of one step on `row`, with the plan's task when it has one, in one of five forms.  n_fused > 0: one of the
// two one-launch forms, which carry the fused populations' update() as well.
// Cursor order: the forms that launch motion and task together advance the cursors BEFORE the launch (fused_task_step
// reads p->step - 1; the task's kernels take the clock after the step) and leave them advanced when the launch fails;
// the plain form advances them after riab_agent_step has returned RIAB_OK.
// action_ready is set by every launch that leaves the coming step's scripted action in the drift buffer and cleared by
// the one that does not (the world's step, until its reset has been launched).
static int motion_stage(RiabPlan* p, float* row, hipStream_t s, int n_fused) {
  int rc;
  if (!p->has_task && n_fused > 0) {  // Agent.update() and the fused populations' update(): one kernel (riab_step1.hip)
    uint32_t mask;
    rc = fused_agent_step(p, row, s, false, &mask, false);
    if (rc) return rc;
    advance_cursors(p, false);
    return RIAB_OK;
  }
  const bool scripted = p->has_task && p->tk.gv_scale > 0.0;
  if (p->has_task && !p->learners.empty()) {
    // a plan with a learner resets LAST (deferred_reset): the task's (or world's) step alone rides with the motion step —
    // no reset, no next action — while the reset counter moves as in every step with auto_reset
    riab::AgentArgs ma;
    rc = riab::fill_agent_args(ma, &p->env, &p->motion, p->state, p->B, p->agent_id0, p->drift, nullptr, nullptr, nullptr,
                               p->seed, p->step, 1, row, p->diag);
    if (rc) return rc;
    advance_cursors(p, true);
    riab::TaskRun t = task_run(p, row);
    t.auto_reset = 0;
    t.gv_x = t.gv_y = nullptr;
    rc = t.world ? riab::launch_motion_world(ma, t, s) : riab::launch_motion_task(ma, t, s);
    if (rc) return rc;
    p->launches += 1;
    p->action_ready = false;
    return RIAB_OK;
  }
  if (n_fused > 0) {  // ... with the task's (or world's) step, its reset and the next action as well (TASK modes)
    advance_cursors(p, true);
    rc = fused_task_step(p, row, s, false);
    if (rc) return rc;
    p->action_ready = scripted;
    return RIAB_OK;
  }
  const bool world = p->has_task && p->tk.world;
  if (world || (p->has_task && riab::g_options[RIAB_OPT_FUSED_TASK] != 0)) {  // (A/B: 0 = motion and task launched separately)
    riab::AgentArgs ma;
    rc = riab::fill_agent_args(ma, &p->env, &p->motion, p->state, p->B, p->agent_id0, p->drift, nullptr, nullptr, nullptr,
                               p->seed, p->step, 1, row, p->diag);
    if (rc) return rc;
    const riab::TaskRun& t = task_run(p, row);
    if (!world) {  // Agent.update() + the rest of TaskEnvironment.step (+ reset, + next action) in one launch
      advance_cursors(p, true);
      rc = riab::launch_motion_task(ma, t, s);
      if (rc) return rc;
      p->launches += 1;
      p->action_ready = scripted;
      return RIAB_OK;
    }
    // Agent.update() + the world's step in one launch, the world's reset in a second: ITS counter moves between the two
    advance_cursors(p, false);
    p->tk.t_env += p->dt_env;
    rc = riab::launch_motion_world(ma, t, s);
    if (rc) return rc;
    p->launches += 1;
    p->action_ready = false;
    if (t.auto_reset) {  // the caller's `if terminal: env.reset()`, decided on the device, and the next scripted action
      p->tk.counter += 1;
      rc = riab_task_world_reset(&p->env, &t.task, t.task_state, t.world, t.task_B, t.agent_id0, t.t_env, t.n_select, t.ordered,
                                 t.seed, t.counter, t.teleport, nullptr, nullptr, t.pos_x, t.pos_y, t.hist_x, t.hist_y, t.ep_log,
                                 t.ep_log_cap, t.ep_count, 1, t.gv_scale, t.gv_x, t.gv_y, t.diag, s);
      if (rc) return rc;
      p->launches += 1;
      p->action_ready = scripted;
    }
    return RIAB_OK;
  }
  // Agent.update(), then the task's launch, if any
  const double* forced = p->forced ? p->forced + p->forced_fill * 2 * p->B : nullptr;
  rc = riab_agent_step(&p->env, &p->motion, p->state, p->B, p->agent_id0, p->drift, nullptr, nullptr, forced, nullptr, p->seed,
                       p->step, 1, row, p->diag, s);
  if (rc) return rc;
  p->launches += 1;
  if (forced) p->forced_fill += 1;
  advance_cursors(p, p->has_task);
  if (p->has_task) {  // the rest of TaskEnvironment.step (+ the caller's `if terminal: reset()`)
    rc = riab::launch_task_fused(task_run(p, row), s);
    if (rc) return rc;
    p->launches += 1;
    p->action_ready = scripted;
  }
  return RIAB_OK;
}

// Neurons.update() of every population the motion stage's launch did not carry, in list order, and every population's
// row cursor: the one place a plan step launches populations.
static int rest_of_populations(RiabPlan* p, const float* row, hipStream_t s, bool skip_fused) {
  for (size_t i = 0; i < p->pops.size(); ++i) {
    if (!skip_fused || !is_fused(p, (int)i)) {
      const int rc = launch_population(p, i, row, s);
      if (rc) return rc;
    }
    if (p->pops[i].capacity_rows > 0) p->pop_fill[i] += 1;
  }
  return RIAB_OK;
}

// What a step with learners needs before anything is launched: every reward bound, and no learner whose row of the step
// (its one scratch row: no history chunk) is zeroed by its reset before another learner has read it
static int check_learners(const RiabPlan* p) {
  for (const PlanLearner& L : p->learners) {
    if (L.reward_kind == RIAB_REWARD_NONE || (L.reward_kind == RIAB_REWARD_TASK && !p->has_task)) return RIAB_EINVAL;
    for (const PlanLearner& M : p->learners) {
      if (M.index >= L.index || p->pops[M.index].capacity_rows > 0) continue;
      const RiabPopulation& q = p->pops[L.index];
      for (int l = 0; l < q.n_inputs; ++l)
        if (q.input_index[l] == M.index) return RIAB_EUNSUPPORTED;
      if (L.reward_kind == RIAB_REWARD_POPULATION && L.reward_index == M.index) return RIAB_EUNSUPPORTED;
    }
  }
  return RIAB_OK;
}

// this step's row of population j, whose cursor points past it
static float* row_of(const RiabPlan* p, int j) {
  const RiabPopulation& q = p->pops[j];
  const int64_t r = q.capacity_rows > 0 ? p->pop_fill[j] - 1 : 0;
  return q.rates_base + r * q.n * p->B;
}

// `learn(reward)` of every learner on the rows the populations have just written and, with a task that resets on its
// own, `reset(lanes = terminal)`: two launches per learner (riab_td_learn_step)
static int learner_stage(RiabPlan* p, hipStream_t s) {
  const uint8_t* const mask = p->has_task && p->tk.auto_reset ? p->tk.terminal_out : nullptr;
  for (const PlanLearner& L : p->learners) {
    const RiabPopulation& q = p->pops[L.index];
    RiabTDLayer layers[RIAB_FF_MAX_INPUTS];
    for (int l = 0; l < q.n_inputs; ++l) {
      layers[l].rates = row_of(p, q.input_index[l]);
      layers[l].trace = L.trace[l];
      layers[l].wt = const_cast<float*>(q.input_wt[l]);
      layers[l].n_in = p->pops[q.input_index[l]].n;
    }
    const void* reward = L.reward;
    int f64 = L.reward_f64;
    int64_t ld_n = L.reward_ld_n, ld_b = L.reward_ld_b;
    if (L.reward_kind == RIAB_REWARD_TASK) {
      reward = p->tk.reward_out;
      f64 = 1;
      ld_n = 0;
      ld_b = 1;
    } else if (L.reward_kind == RIAB_REWARD_POPULATION) {
      reward = row_of(p, L.reward_index);
      f64 = 0;
      ld_n = p->B;
      ld_b = 1;
    }
    const int rc = riab_td_learn_step(&L.p, layers, q.n_inputs, reward, f64, ld_n, ld_b, row_of(p, L.index), L.v_last, L.dvdt,
                                      q.rates_prime, L.td, mask, q.capacity_rows == 0 ? 1 : 0, L.workspace, L.workspace_floats, s);
    if (rc) return rc;
    p->launches += (L.p.n > 256 ? 3 : 2);
  }
  return RIAB_OK;
}

// the reset a plan with a learner left for last: the caller's `env.reset(mask = terminal)`, decided on the device, on the
// newest history row; the coming step's scripted action is first_action's (the world's reset writes it itself)
static int deferred_reset(RiabPlan* p, float* row, hipStream_t s) {
  if (!p->has_task || !p->tk.auto_reset) return RIAB_OK;
  const riab::TaskRun& t = task_run(p, row);
  int rc;
  if (t.world) {
    rc = riab_task_world_reset(&p->env, &t.task, t.task_state, t.world, t.task_B, t.agent_id0, t.t_env, t.n_select, t.ordered,
                               t.seed, t.counter, t.teleport, nullptr, nullptr, t.pos_x, t.pos_y, t.hist_x, t.hist_y, t.ep_log,
                               t.ep_log_cap, t.ep_count, 1, t.gv_scale, t.gv_x, t.gv_y, t.diag, s);
    if (rc == RIAB_OK) p->action_ready = t.gv_scale > 0.0;
  } else {
    rc = riab_task_reset(&p->env, &t.task, t.task_state, t.terminal_out, t.task_B, t.agent_id0, t.t_env, t.n_select, t.ordered,
                         t.seed, t.counter, t.teleport, nullptr, nullptr, t.pos_x, t.pos_y, t.hist_x, t.hist_y, t.ep_log,
                         t.ep_log_cap, t.ep_count, t.diag, s);
  }
  if (rc == RIAB_OK) p->launches += 1;
  return rc;
}

extern "C" int riab_plan_step(RiabPlan* p, int32_t n_steps, riab_stream_t stream) {
  if (!p || n_steps <= 0) return RIAB_EINVAL;
  if (!p->learners.empty()) {
    const int rc = check_learners(p);
    if (rc) return rc;
  }
  if (riab_plan_rows_free(p) < n_steps) return RIAB_EFULL;
  if (p->forced && (p->has_task || p->forced_rows - p->forced_fill < n_steps)) return p->has_task ? RIAB_EINVAL : RIAB_EFULL;
  hipStream_t s = (hipStream_t)stream;
  p->pre_pending.assign(p->pops.size(), 0);
  const int n_fused = plan_fused(p, true);
  for (int32_t k = 0; k < n_steps; ++k) {
    float* row = p->hist_base ? p->hist_base + p->hist_fill * (int64_t)RIAB_HIST_ROWS * p->B : p->row_scratch;
    int rc = p->has_task && p->tk.gv_scale > 0.0 ? first_action(p, s) : RIAB_OK;
    if (!rc) rc = motion_stage(p, row, s, n_fused);
    if (!rc) rc = rest_of_populations(p, row, s, n_fused > 0);
    if (!rc && !p->learners.empty()) {  // learn, then reset
      rc = learner_stage(p, s);
      if (!rc) rc = deferred_reset(p, row, s);
    }
    if (rc) return rc;
  }
  return RIAB_OK;
}
