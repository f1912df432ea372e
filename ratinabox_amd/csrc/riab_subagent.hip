// contribs.SubAgent on gfx950, second part (reference contribs/SubAgent.py:118-179, 358-432): the DumbAgent's step — a
// wrong position that wanders on a spring round the lead — and the ReplayAgent's — the lead's position, except while the
// lane explores somewhere else at replay speed.  One lane = one agent; every array is [rows][B] with the agent axis
// fastest; blocks of 64 threads.  Nothing here talks to another workgroup.
#include "riab_agent_kernel.h"

namespace riab {

#define RIAB_TAG_DUMB 0x44554D42u  // the Philox stream of the DumbAgent's normals

struct DumbArgs {
  const double* lead;  // the lead's state [RIAB_STATE_ROWS][B]
  double* disp;        // [2][B]
  double* vel;         // [2][B]
  double* out;         // [2][B]
  double dt, theta, sigma, accel;
  int64_t n_agents;    // lanes below it are real agents: only they are counted in diag
  int32_t* diag;
};

// `a` carries what the motion kernel's helpers read: the walls, the shape, the extent, the Philox key, the step and
// the normals (z_in / z_out [2][B])
template <int IN>
__global__ __launch_bounds__(64) void dumb_agent_step_kernel(const AgentArgs a, const DumbArgs d) {
  RIAB_EXACT_FP
  const int lane = (int)threadIdx.x;
  __shared__ Wall<double> s_w[RIAB_MAX_WALLS];
  stage_walls<double>(a, s_w, lane, 64);
  __syncthreads();
  const int64_t B = a.B;
  const int64_t b = (int64_t)blockIdx.x * 64 + lane;
  if (b >= B) return;
  const uint32_t aid = (uint32_t)(a.agent_id0 + b);
  const double lx = d.lead[RIAB_S_POS_X * B + b], ly = d.lead[RIAB_S_POS_Y * B + b];
  double dx = d.disp[b], dy = d.disp[B + b];
  double vx = d.vel[b], vy = d.vel[B + b];
  // ---- the step's two standard normals
  double z0, z1;
  if (IN == 1) {
    z0 = a.z_in[b];
    z1 = a.z_in[B + b];
  } else {
    const u32x4 w = philox4x32_10((uint32_t)a.step0, (uint32_t)(a.step0 >> 32), aid, RIAB_TAG_DUMB, a.k0, a.k1);
    const float u1 = ((float)(w.x >> 8) + 0.5f) * 0x1.0p-24f, u2 = (float)(w.y >> 8) * 0x1.0p-24f;
    const float rr = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));  // sqrt(-2 ln u1)
    z0 = (double)(rr * __builtin_amdgcn_cosf(u2));
    z1 = (double)(rr * __builtin_amdgcn_sinf(u2));
  }
  if (a.z_out) {
    a.z_out[b] = z0;
    a.z_out[B + b] = z1;
  }
  // ---- the displacement velocity under stochastic + spring dynamics, then the displacement (SubAgent.py:154-163)
  {
    const double ou_x = d.theta * (0.0 - vx) * d.dt + d.sigma * (d.dt * z0);
    const double ou_y = d.theta * (0.0 - vy) * d.dt + d.sigma * (d.dt * z1);
    const double sp_x = (-d.accel) * dx * d.dt, sp_y = (-d.accel) * dy * d.dt;
    vx += ou_x + sp_x;
    vy += ou_y + sp_y;
    dx += vx * d.dt;
    dy += vy * d.dt;
  }
  // ---- the spring against every wall (SubAgent.py:167-173; utils.vector_intercepts: list a the walls, list b the
  // segment lead -> lead + displacement, the quotients themselves: the smallest one scales the displacement)
  int n_cut = 0;
  {
    const double ex = lx + dx, ey = ly + dy;
    const double sbx = ex - lx, sby = ey - ly;
    double l_min = INFINITY;
    for (int w = 0; w < a.n_walls; ++w) {
      const Wall<double> W = s_w[w];
      const double d0x = lx - W.ax, d0y = ly - W.ay;
      const double l_a = (d0x * (-sby) + d0y * sbx) / (W.sx * (-sby) + W.sy * sbx);
      const double l_b = ((-d0x) * (-W.sy) + (-d0y) * W.sx) / (sbx * (-W.sy) + sby * W.sx);
      if (l_a > 0.0 && l_a < 1.0 && l_b > 0.0 && l_b < 1.0) l_min = l_b < l_min ? l_b : l_min;
    }
    if (l_min < INFINITY) {
      const double f = 0.95 * l_min;
      dx *= f;
      dy *= f;
      n_cut = 1;
    }
  }
  // ---- strict boundary conditions on lead + displacement (SubAgent.py:175-177): the motion kernel's own safety net
  double px = lx + dx, py = ly + dy;
  int n_bc = 0, n_sat = 0;
  {
    MotionConst<double> k;
    motion_const_scalars<double>(k, a);  // (the extent and the shape are what boundary_net reads)
    boundary_net<double>(k, a, s_w, 0, b, aid, px, py, n_bc, n_sat);
  }
  // ---- the displacement as the environment sees it (SubAgent.py:178): periodic-aware
  step_displacement<double>(a, px, py, lx, ly, dx, dy);
  d.disp[b] = dx;
  d.disp[B + b] = dy;
  d.vel[b] = vx;
  d.vel[B + b] = vy;
  d.out[b] = px;
  d.out[B + b] = py;
  if (d.diag && b < d.n_agents) {
    if (n_cut) atomicAdd(d.diag + RIAB_DUMB_DIAG_WALL_CUTS, n_cut);
    if (n_bc) atomicAdd(d.diag + RIAB_DUMB_DIAG_BOUNDARY, n_bc);
    if (n_sat) atomicAdd(d.diag + RIAB_DUMB_DIAG_SATURATIONS, n_sat);
  }
}

// ---- ReplayAgent (SubAgent.py:358-432) -----------------------------------------------------------------------------
// The reference rolls a replay's whole trajectory out when it starts and interpolates that table on the following
// steps, at a query distance speed * (t - start) that only grows.  The interpolated point needs the two records that
// bracket the query, so the lane keeps those two and its sham agent is advanced — agent_step_body itself, one step per
// call on the sham agent's state rows, as in theta_sequence_rollout_kernel — only until its newest record reaches the
// query of this call.  A wave leaves the loop when none of its lanes needs another step; a lane that needs none (or is
// in no replay at all) keeps stepping with its wave (the motion step takes wave-uniform decisions: a lane must see the
// wave a plain launch would show it), but its state and records of the moment are what is written back.
#define RIAB_TAG_REPLAY 0x5245504Cu  // the Philox streams of the ReplayAgent's draws (^ 2: the start position's sampler)

struct ReplayArgs {
  const double* lead;  // the lead's state [RIAB_STATE_ROWS][B]
  int32_t* flag;       // [B]
  double* rp;          // [RIAB_REPLAY_ROWS][B]
  double t, freq_dt, mean_speed, mean_duration, speed_mean;
  const double* draws_in;  // [RIAB_REPLAY_DRAWS][B] or null
  double* draws_out;       // [RIAB_REPLAY_DRAWS][B] or null
  uint32_t k0, k1;         // the ReplayAgent's own Philox key ...
  uint64_t step;           // ... and step
  int K;
  double* out;         // [2][B]
  int32_t* steps;      // [B]
  int32_t* diag;
  int64_t n_agents;
};

template <int IN>
__global__ __launch_bounds__(64) void replay_agent_step_kernel(const AgentArgs a_in, const ReplayArgs r) {
  RIAB_EXACT_FP
  const int64_t B = a_in.B;
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool valid = b < B;
  double* const st = a_in.state + (valid ? b : 0);
  double* const rp = r.rp + (valid ? b : 0);
  double fin[RIAB_STATE_ROWS];
  double speed = 0.0, t_start = 0.0, t_end = 0.0, d_start = 0.0;
  double lo_d = 0.0, lo_x = 0.0, lo_y = 0.0, hi_d = 0.0, hi_x = 0.0, hi_y = 0.0;
  double query = 0.0, px = 0.0, py = 0.0;
  int flag = 0, n_started = 0, n_ended = 0, n_resat = 0;
  bool moving = false;  // in a replay that goes on: the position is interpolated
  if (valid) {
#pragma unroll
    for (int i = 0; i < RIAB_STATE_ROWS; ++i) fin[i] = st[i * B];
    const double lx = r.lead[RIAB_S_POS_X * B + b], ly = r.lead[RIAB_S_POS_Y * B + b];
    px = lx;
    py = ly;
    flag = r.flag[b];
    speed = rp[RIAB_RP_SPEED * B];
    t_start = rp[RIAB_RP_T_START * B];
    t_end = rp[RIAB_RP_T_END * B];
    d_start = rp[RIAB_RP_D_START * B];
    lo_d = rp[(RIAB_RP_LO + 0) * B]; lo_x = rp[(RIAB_RP_LO + 1) * B]; lo_y = rp[(RIAB_RP_LO + 2) * B];
    hi_d = rp[(RIAB_RP_HI + 0) * B]; hi_x = rp[(RIAB_RP_HI + 1) * B]; hi_y = rp[(RIAB_RP_HI + 2) * B];
    const double nan = __builtin_nan("");
    double dr[RIAB_REPLAY_DRAWS] = {nan, nan, nan, nan, nan, nan};
    if (!flag) {
      // ---- not in a replay: the trigger, then the four draws of a start (SubAgent.py:392-407)
      const uint32_t aid = (uint32_t)(a_in.agent_id0 + b);
      u32x4 w = {0u, 0u, 0u, 0u};
      if (!r.draws_in) w = philox4x32_10((uint32_t)r.step, (uint32_t)(r.step >> 32), aid, RIAB_TAG_REPLAY, r.k0, r.k1);
      const double u = r.draws_in ? r.draws_in[RIAB_RD_U * B + b] : (double)u01_24(w.x);
      dr[RIAB_RD_U] = u;
      if (!(u > r.freq_dt)) {
        double sx, sy, direction, duration;
        if (r.draws_in) {
          speed = r.draws_in[RIAB_RD_SPEED * B + b];
          duration = r.draws_in[RIAB_RD_DURATION * B + b];
          sx = r.draws_in[RIAB_RD_POS_X * B + b];
          sy = r.draws_in[RIAB_RD_POS_Y * B + b];
          direction = r.draws_in[RIAB_RD_DIRECTION * B + b];
        } else {
          // Rayleigh(scale) = scale * sqrt(-2 ln(1 - U)); U in [0, 1): the logarithm's argument is never 0
          speed = r.mean_speed * sqrt(-2.0 * log(1.0 - (double)u01_24(w.y)));
          duration = r.mean_duration * sqrt(-2.0 * log(1.0 - (double)u01_24(w.z)));
          direction = 6.283185307179586 * (double)u01_24(w.w);
          // uniform over the extent, rejected until inside (Environment.sample_positions(1, "random")): the bounded
          // sampler of the motion kernel's resample boundary condition, on this agent's own stream
          // (the edges are read straight from the wall table: starts are rare)
          auto edge = [&](int kk, double& ax, double& ay, double& bx, double& by) {
            ax = a_in.walls[4 * kk]; ay = a_in.walls[4 * kk + 1]; bx = a_in.walls[4 * kk + 2]; by = a_in.walls[4 * kk + 3];
          };
          int attempt = 0;
          sx = sy = 0.0;
          for (; attempt < RIAB_MAX_RESAMPLES; ++attempt) {
            const u32x4 v = philox4x32_10((uint32_t)r.step, (uint32_t)(r.step >> 32) ^ ((uint32_t)attempt << 24), aid,
                                          RIAB_TAG_REPLAY ^ 2u, r.k0, r.k1);
            sx = uniform_between(a_in.shape.e0, a_in.shape.e1, u01_24(v.x));
            sy = uniform_between(a_in.shape.e2, a_in.shape.e3, u01_24(v.y));
            if (env_contains(a_in.shape, sx, sy, edge)) break;
          }
          if (attempt == RIAB_MAX_RESAMPLES) n_resat = 1;
        }
        dr[RIAB_RD_SPEED] = speed;
        dr[RIAB_RD_DURATION] = duration;
        dr[RIAB_RD_POS_X] = sx;
        dr[RIAB_RD_POS_Y] = sy;
        dr[RIAB_RD_DIRECTION] = direction;
        const double half = r.mean_duration / 2;
        duration = duration > half ? duration : half;  // max(draw, mean / 2)
        t_start = r.t;
        t_end = r.t + duration;
        // ReplayAgent.initialise_position_and_velocity (Agent.py:523-531)
        double sn, cs;
        sincos(direction, &sn, &cs);
        fin[RIAB_S_POS_X] = sx;
        fin[RIAB_S_POS_Y] = sy;
        fin[RIAB_S_VEL_X] = r.speed_mean * cs;
        fin[RIAB_S_VEL_Y] = r.speed_mean * sn;
        fin[RIAB_S_ROT_VEL] = 0.0;
        d_start = fin[RIAB_S_DIST];
        lo_d = hi_d = 0.0;
        lo_x = hi_x = sx;
        lo_y = hi_y = sy;
        px = sx;
        py = sy;
        flag = 1;
        n_started = 1;
      }
    } else if (r.t < t_end) {
      query = speed * (r.t - t_start);
      moving = true;
    } else {
      flag = 0;
      n_ended = 1;
    }
    if (r.draws_out) {
#pragma unroll
      for (int i = 0; i < RIAB_REPLAY_DRAWS; ++i) r.draws_out[i * B + b] = dr[i];
    }
  }
  // ---- the sham agent, as far as this call's query needs
  bool active = moving && !(hi_d >= query);
  int n = 0;
  AgentArgs a = a_in;
  for (int k = 0; k < r.K; ++k) {
    if (__builtin_amdgcn_ballot_w64(active) == 0) break;
    a.step0 = a_in.step0 + (uint64_t)k;
    a.z_in = a_in.z_in ? a_in.z_in + (int64_t)k * 2 * B : nullptr;
    a.z_out = a_in.z_out ? a_in.z_out + (int64_t)k * 2 * B : nullptr;
    agent_step_body<double, IN, false>(a);
    if (active) {
#pragma unroll
      for (int i = 0; i < RIAB_STATE_ROWS; ++i) fin[i] = st[i * B];
      lo_d = hi_d; lo_x = hi_x; lo_y = hi_y;
      hi_d = fin[RIAB_S_DIST] - d_start;
      hi_x = fin[RIAB_S_POS_X];
      hi_y = fin[RIAB_S_POS_Y];
      n = k + 1;
      active = !(hi_d >= query);
    }
  }
  if (!valid) return;
#pragma unroll
  for (int i = 0; i < RIAB_STATE_ROWS; ++i) st[i * B] = fin[i];
  if (moving) {
    if (active) {  // out of steps: the newest record
      px = hi_x;
      py = hi_y;
    } else {       // interp1d's rounding: the slope, then slope * (x - x_lo) + y_lo
      const double run = hi_d - lo_d, along = query - lo_d;
      const double s0 = (hi_x - lo_x) / run, s1 = (hi_y - lo_y) / run;
      px = s0 * along + lo_x;
      py = s1 * along + lo_y;
    }
  }
  r.flag[b] = flag;
  rp[RIAB_RP_SPEED * B] = speed;
  rp[RIAB_RP_T_START * B] = t_start;
  rp[RIAB_RP_T_END * B] = t_end;
  rp[RIAB_RP_D_START * B] = d_start;
  rp[(RIAB_RP_LO + 0) * B] = lo_d; rp[(RIAB_RP_LO + 1) * B] = lo_x; rp[(RIAB_RP_LO + 2) * B] = lo_y;
  rp[(RIAB_RP_HI + 0) * B] = hi_d; rp[(RIAB_RP_HI + 1) * B] = hi_x; rp[(RIAB_RP_HI + 2) * B] = hi_y;
  r.out[b] = px;
  r.out[B + b] = py;
  r.steps[b] = n;
  if (r.diag && b < r.n_agents) {
    if (n_started) atomicAdd(r.diag + RIAB_REPLAY_DIAG_STARTED, 1);
    if (n_ended) atomicAdd(r.diag + RIAB_REPLAY_DIAG_ENDED, 1);
    if (moving && active) atomicAdd(r.diag + RIAB_REPLAY_DIAG_SATURATIONS, 1);
    if (n_resat) atomicAdd(r.diag + RIAB_REPLAY_DIAG_RESAMPLE, 1);
  }
}

}  // namespace riab

using namespace riab;

extern "C" int riab_replay_agent_step(const RiabEnv* env, const RiabMotion* motion, const double* lead_state, double* sham_state,
                                      int64_t B, int64_t n_agents, int64_t agent_id0, int32_t* flag, double* replay_state,
                                      double t, double freq_dt, double mean_speed, double mean_duration, double speed_mean,
                                      const double* draws_in, double* draws_out, uint64_t seed, uint64_t step,
                                      const double* z_in, double* z_out, uint64_t sham_seed, uint64_t sham_step0, int32_t K,
                                      double* pos_out, int32_t* steps_taken, int32_t* motion_diag, int32_t* diag,
                                      riab_stream_t stream) {
  if (!env || !motion || !lead_state || !sham_state || !flag || !replay_state || !pos_out || !steps_taken) return RIAB_EINVAL;
  if (K < 1 || B <= 0 || n_agents < 0 || n_agents > B) return RIAB_EINVAL;
  if (B % 4 != 0) return RIAB_EALIGN;
  if (motion->has_drift || !(motion->dt > 0.0)) return RIAB_EINVAL;
  AgentArgs a;
  const int rc = fill_agent_args(a, env, motion, sham_state, B, agent_id0, nullptr, z_in, z_out, nullptr, sham_seed, sham_step0, 1,
                                 nullptr, motion_diag);
  if (rc) return rc;
  ReplayArgs r;
  r.lead = lead_state;
  r.flag = flag;
  r.rp = replay_state;
  r.t = t;
  r.freq_dt = freq_dt;
  r.mean_speed = mean_speed;
  r.mean_duration = mean_duration;
  r.speed_mean = speed_mean;
  r.draws_in = draws_in;
  r.draws_out = draws_out;
  r.k0 = (uint32_t)seed;
  r.k1 = (uint32_t)(seed >> 32);
  r.step = step;
  r.K = K;
  r.out = pos_out;
  r.steps = steps_taken;
  r.diag = diag;
  r.n_agents = n_agents;
  const dim3 grid((unsigned)((B + 63) / 64)), block(64);
  if (z_in) hipLaunchKernelGGL(replay_agent_step_kernel<1>, grid, block, 0, (hipStream_t)stream, a, r);
  else hipLaunchKernelGGL(replay_agent_step_kernel<0>, grid, block, 0, (hipStream_t)stream, a, r);
  return (int)hipGetLastError();
}

extern "C" int riab_dumb_agent_step(const RiabEnv* env, const double* lead_state, int64_t B, int64_t n_agents, int64_t agent_id0,
                                    double* displacement, double* velocity, double dt, double theta, double sigma,
                                    double acceleration_scale, const double* z_in, double* z_out, uint64_t seed, uint64_t step,
                                    double* pos_out, int32_t* diag, riab_stream_t stream) {
  if (!env || !lead_state || !displacement || !velocity || !pos_out || B <= 0 || n_agents < 0 || n_agents > B) return RIAB_EINVAL;
  if (!(dt > 0.0)) return RIAB_EINVAL;
  if (B % 4 != 0) return RIAB_EALIGN;
  RiabMotion none = {};  // (no motion model here: the argument block is filled for its environment, key and normals)
  none.dt = dt;
  AgentArgs a;
  const int rc = fill_agent_args(a, env, &none, displacement, B, agent_id0, nullptr, z_in, z_out, nullptr, seed, step, 1, nullptr,
                                 nullptr);
  if (rc) return rc;
  DumbArgs d;
  d.lead = lead_state;
  d.disp = displacement;
  d.vel = velocity;
  d.out = pos_out;
  d.dt = dt;
  d.theta = theta;
  d.sigma = sigma;
  d.accel = acceleration_scale;
  d.n_agents = n_agents;
  d.diag = diag;
  const dim3 grid((unsigned)((B + 63) / 64)), block(64);
  if (z_in) hipLaunchKernelGGL(dumb_agent_step_kernel<1>, grid, block, 0, (hipStream_t)stream, a, d);
  else hipLaunchKernelGGL(dumb_agent_step_kernel<0>, grid, block, 0, (hipStream_t)stream, a, d);
  return (int)hipGetLastError();
}
