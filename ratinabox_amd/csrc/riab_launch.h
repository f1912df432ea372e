// Host launchers that one translation unit defines and another calls, and the two records the step plan hands them.
// Included by the defining AND the calling translation unit: the library is linked with -shared, where a prototype that
// has drifted from its definition shows only when the library is loaded — here it fails to compile.  Host code only.
#pragma once

#include "riab_device.h"

namespace riab {

struct AgentArgs;  // riab_agent_kernel.h: the motion kernel's argument block

// What a step plan holds about its task (riab_plan_set_task, riab_plan_set_task_world) and the values of one call: the
// arguments of TaskEnvironment.step + the caller's `if terminal: reset()` + the next scripted action.
struct TaskRun {
  const RiabEnv* env;
  RiabTask task;
  double* task_state;
  int64_t task_B;
  double *pos_x, *pos_y;  // the agents' positions: rows of the float64 state
  double* reward_out;
  uint8_t* terminal_out;
  int32_t* diag;
  int32_t auto_reset, n_select, ordered, teleport;
  int64_t agent_id0;
  uint64_t seed;
  double* ep_log;
  int64_t ep_log_cap;
  int32_t* ep_count;
  double gv_scale;  // speed of the scripted action (<= 0: the caller acts)
  double* world;    // the lanes are the agents of ONE world (null: every lane its own replica), and its scratch:
  uint64_t* world_met;
  int32_t *world_cand, *world_ctl;
  // per call
  double t_env;            // the task's clock after this step
  uint64_t counter;        // the reset's RNG counter
  float *hist_x, *hist_y;  // the history row a teleport patches (null: the launch writes its row itself)
  double *gv_x, *gv_y;     // where the coming step's scripted action goes (null: none)
};

// Rows [rate_row, rate_row + T) of population pops[index] from T history rows: what riab_plan.hip (one row per step) and
// riab_simulate.hip (a chunk of rows) fill in for launch_population_rows.
struct PopRows {
  const RiabEnv* env;
  const RiabPopulation* pops;
  int index;
  const float* hist;  // the first history row, [RIAB_HIST_ROWS][B] ...
  int64_t hist_ld;    // ... and the distance to the next one, in elements
  int64_t B;
  int32_t T;
  int64_t rate_row;
  float dt;
  uint64_t seed, step0;  // step0: Agent.update() calls made when the first row's Neurons.update() runs
  int64_t agent_id0;
  const double* state;     // the float64 state, for the kinds that read Agent.velocity from it (null: those are refused) ...
  double clock;            // ... and Agent.t
  uint32_t* xch_arrivals;  // boundary vector cells: the ray exchange's arrival count (null: no exchange) ...
  int n_cus;               // ... and the compute units its launches count on
  const int64_t* cursors;  // FeedForwardLayer: per population, the cursor PAST the row written this step (null: inputs at rate_row)
  bool write_prime;        // FeedForwardLayer: rates_prime is written
};

// riab_plan.hip
int launch_population_rows(const PopRows& r, hipStream_t s, int64_t* launches);
int check_population(const RiabPopulation& q, int n_before);
// an assigned RIAB_POP_* value (riab_hip.h: 10 is not one)
inline bool population_kind_known(int kind) {
  return (kind >= RIAB_POP_PLACE && kind <= RIAB_POP_THETA_PLACE) || kind == RIAB_POP_PLANE_WAVE;
}

// riab_agent.hip
int launch_agent_pub(const AgentArgs& a, hipStream_t s, bool* state_published);
int launch_agent_forced(const AgentArgs& a, hipStream_t s);
int launch_agent_plain(const AgentArgs& a, hipStream_t s);
int traj_kernel_regs();
int launch_motion_task(const AgentArgs& ma, const TaskRun& t, hipStream_t s);

// riab_task.hip, riab_task_world.hip
int launch_task_fused(const TaskRun& t, hipStream_t s);
int launch_motion_world(const AgentArgs& ma, const TaskRun& t, hipStream_t s);

// riab_step1.hip: the one-launch step
int step1_supported(const RiabEnv* env, const RiabPopulation* pop, int64_t B);
int launch_step1(const AgentArgs& a, const RiabEnv* env, const Step1PopRef* refs, int n_pops, uint64_t seed, uint64_t step_after,
                 uint32_t* sync_words, uint32_t epoch, bool* walls_ready, int n_cus, hipStream_t s, bool query);
int launch_step1_task(const AgentArgs& a, const RiabEnv* env, const Step1PopRef* refs, int n_pops, uint64_t seed,
                      uint64_t step_after, uint32_t* sync_words, uint32_t epoch, bool* walls_ready, int n_cus, const TaskRun& t,
                      hipStream_t s, bool query);

// riab_bvc.hip: boundary vector cells with the ray exchange of one-row launches
int launch_bvc(const RiabEnv* env, const RiabRateIO* io, const double* test_dirs, const double* ray_rden, int32_t K,
               const float* cells, const float* vm_table, const float* inv_norm, int32_t n, int32_t egocentric,
               float* ray_out, const int32_t* cell_rows, const int32_t* windows, float* xch, uint32_t* xch_count,
               uint32_t* xch_arrivals, int n_cus, hipStream_t stream);

// riab_td.hip: the checks of every riab_td_* entry point on a learner's constants and layers
int td_check(const RiabTDParams* p, const RiabTDLayer* layers, int32_t n_layers);

// riab_ovc.hip: the most objects the vector-cell kernel's LDS staging holds (-1: no device)
int ovc_object_limit();

// riab_rates.hip: the flag-coupled rate stage of riab_simulate
int stream_supported(const RiabEnv* env, const RiabPopulation* pop, int64_t B);
int launch_rate_stream(const RiabEnv* env, const RiabPopulation* pop, const float* hist, int64_t B, int32_t T, float dt,
                       uint64_t seed, uint64_t step0, int64_t agent_id0, uint32_t* ctrl, uint32_t spin_limit, bool stamps,
                       hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop, bool dry_run, bool reserve,
                       uint32_t serial_rows);
int launch_stream_gate(uint32_t* ctrl, uint32_t started_target, uint32_t n_traj, uint32_t progress_target,
                       uint32_t spin_limit, bool sleep_long, uint32_t final_target, hipStream_t s);
int launch_stream_open(uint32_t* ctrl, uint32_t n_traj, uint32_t step_base, hipStream_t s);

}  // namespace riab
