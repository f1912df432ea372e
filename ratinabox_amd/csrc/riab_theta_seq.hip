// contribs.SubAgent on gfx950 (reference contribs/SubAgent.py): the position of a ThetaSequenceAgent — NaN, a point of
// the lead's own past, or a point of a freshly simulated future — once per step, the forward rollout that makes that
// future once per theta cycle, and the ShiftAgent's one-line position.  One lane = one agent; every array is
// [rows][B] with the agent axis fastest.  Nothing here talks to another workgroup.
#include "riab_agent_kernel.h"

namespace riab {

// ---- scipy.interpolate.interp1d(x, y, axis=0) with its default arguments, restated ---------------------------------
// (kind="linear", bounds_error=True, assume_sorted=False: the abscissae here are distances travelled, non-decreasing,
// so its stable argsort is the identity.)  _call_linear: i = searchsorted(x, x_new) [side="left"], clipped to
// [1, n - 1]; slope = (y[i] - y[i-1]) / (x[i] - x[i-1]); y_new = slope * (x_new - x[i-1]) + y[i-1].  `i_left` is the
// searchsorted index.  Every operation rounded on its own, as NumPy does.
template <class X, class Y>
__device__ __forceinline__ void interp1d_linear(int n, int i_left, double x_new, X xs, Y ys, double& ox, double& oy) {
  RIAB_EXACT_FP
  int i = i_left < 1 ? 1 : (i_left > n - 1 ? n - 1 : i_left);
  const double x_lo = xs(i - 1), x_hi = xs(i);
  double y0_lo, y1_lo, y0_hi, y1_hi;
  ys(i - 1, y0_lo, y1_lo);
  ys(i, y0_hi, y1_hi);
  const double run = x_hi - x_lo, along = x_new - x_lo;
  const double s0 = (y0_hi - y0_lo) / run, s1 = (y1_hi - y1_lo) / run;
  ox = s0 * along + y0_lo;
  oy = s1 * along + y1_lo;
}
// np.searchsorted(x, v) (side="left") over n non-decreasing values: the first index whose value is >= v
template <class X>
__device__ __forceinline__ int lower_bound(int n, double v, X xs) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (xs(mid) < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct ThetaStepArgs {
  const double* lead;    // the lead's state [RIAB_STATE_ROWS][B]
  int64_t B;
  int64_t n_agents;     // lanes below it are real agents: only they are counted in diag
  double* ring;          // [capacity][3][B]: (distance travelled, x, y) of the lead after each of its steps
  int capacity, lookback;
  int64_t n_before;      // records appended before this call
  int branch;
  double phase, d_half, theta_frac;
  const double* future;  // [K + 1][3][B]
  const int32_t* count;  // [B]
  int K;
  double scale;
  int periodic;
  double* out;           // [2][B]
  int32_t* diag;
};

__global__ __launch_bounds__(64) void theta_sequence_step_kernel(const ThetaStepArgs a) {
  RIAB_EXACT_FP
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const int64_t B = a.B;
  const double lx = a.lead[RIAB_S_POS_X * B + b], ly = a.lead[RIAB_S_POS_Y * B + b], ld = a.lead[RIAB_S_DIST * B + b];
  // ---- the record of this step (SubAgent.py:259-264): the slot is the same for every lane, three coalesced rows
  const int slot_new = (int)(a.n_before % a.capacity);
  double* const rec = a.ring + (int64_t)slot_new * 3 * B + b;
  rec[0] = ld;
  rec[B] = lx;
  rec[2 * B] = ly;
  const double nan = __builtin_nan("");
  double px = nan, py = nan;
  int n_raise_behind = 0, n_raise_ahead = 0, n_far = 0;
  if (a.branch == RIAB_THETA_BEHIND) {
    // ---- look behind (SubAgent.py:274-300)
    if (ld < a.d_half) {
      px = lx;
      py = ly;
    } else {
      // the window: the newest min(lookback, records) records, this step's among them (:283-286)
      const int64_t n_rec = a.n_before + 1;
      const int L = (int)(n_rec < (int64_t)a.lookback ? n_rec : (int64_t)a.lookback);
      const int slot0 = (int)((n_rec - L) % a.capacity);
      auto row = [&](int i) -> const double* {
        int s = slot0 + i;
        s = s >= a.capacity ? s - a.capacity : s;
        return a.ring + (int64_t)s * 3 * B + b;
      };
      auto dist = [&](int i) -> double { return i == L - 1 ? ld : row(i)[0]; };
      const double c = a.d_half / a.theta_frac, m = -2 * c;
      const double back = m * a.phase + c;
      const double x = ld - back;
      // idx = np.argmin(np.abs(true_distances - x)) (:295): the distances do not decrease, so |d - x| falls and then
      // rises — the minimum sits beside the first record at or beyond x, and NumPy returns the FIRST index among equals
      auto err = [&](int i) -> double { return fabs(dist(i) - x); };
      const int lb = lower_bound(L, x, dist);
      int idx = lb >= L ? L - 1 : lb;
      while (idx > 0 && err(idx - 1) <= err(idx)) --idx;
      // true_distances[idx - 3 : idx + 3] (:297-298) by Python's slice rules: a negative start counts from the end
      int start = idx - 3;
      if (start < 0) {
        start += L;
        start = start < 0 ? 0 : start;
      }
      const int stop = idx + 3 < L ? idx + 3 : L;
      const int n = stop - start;
      auto xs = [&](int j) -> double { return dist(start + j); };
      auto ys = [&](int j, double& y0, double& y1) {
        const double* r = row(start + j);
        y0 = r[B];
        y1 = r[2 * B];
      };
      // where interp1d raises (fewer than two points: the empty slice of idx < 3; x outside the points): NaN, counted
      if (n < 2 || x < xs(0) || x > xs(n - 1)) {
        ++n_raise_behind;
      } else {
        int i_left = 0;
        for (int j = 0; j < n; ++j) i_left += xs(j) < x ? 1 : 0;
        interp1d_linear(n, i_left, x, xs, ys, px, py);
      }
    }
  } else if (a.branch == RIAB_THETA_AHEAD) {
    // ---- look ahead (SubAgent.py:328-334) in the lane's future table (riab_theta_sequence_rollout)
    const double c = -a.d_half / a.theta_frac, m = -2 * c;
    const double ahead = m * a.phase + c;
    const double x = ld + ahead;
    const int cnt = a.count[b];
    const int n = cnt + 1;
    auto xs = [&](int j) -> double { return a.future[((int64_t)j * 3 + 0) * B + b]; };
    auto ys = [&](int j, double& y0, double& y1) {
      y0 = a.future[((int64_t)j * 3 + 1) * B + b];
      y1 = a.future[((int64_t)j * 3 + 2) * B + b];
    };
    if (cnt < 1 || cnt > a.K || x < xs(0) || x > xs(n - 1)) ++n_raise_ahead;
    else interp1d_linear(n, lower_bound(n, x, xs), x, xs, ys, px, py);
  }
  // ---- further than d_half from the lead (the periodic wrap included): no position (SubAgent.py:341-343)
  {
    double dx = px - lx, dy = py - ly;
    if (a.periodic) {
      const double hs = a.scale / 2;
      if (fabs(dx) > hs) dx = -copysign(a.scale - fabs(dx), dx);
      if (fabs(dy) > hs) dy = -copysign(a.scale - fabs(dy), dy);
    }
    const double far = sqrt(dx * dx + dy * dy);
    if (far > a.d_half) {  // (false for NaN)
      px = nan;
      py = nan;
      ++n_far;
    }
  }
  a.out[b] = px;
  a.out[B + b] = py;
  if (a.diag && b < a.n_agents) {
    if (n_raise_behind) atomicAdd(a.diag + RIAB_THETA_DIAG_BEHIND, n_raise_behind);
    if (n_raise_ahead) atomicAdd(a.diag + RIAB_THETA_DIAG_AHEAD, n_raise_ahead);
    if (n_far) atomicAdd(a.diag + RIAB_THETA_DIAG_FAR, n_far);
  }
}

// ---- the forward rollout (SubAgent.py:305-327) ---------------------------------------------------------------------
// The lane's ForwardSequenceAgent takes the lead's position, velocity, rotational velocity and distance, and is advanced
// by the motion model — agent_step_body itself, one step per call on the ForwardSequenceAgent's state rows, so a rollout
// step IS a riab_agent_step(T = 1) step — until it has covered `forward_distance`; every step's (distance, x, y) goes
// into the lane's future table.  A wave leaves the loop when all its lanes are there; a lane that arrives earlier keeps
// stepping with its wave (the motion step takes wave-uniform decisions, e.g. which sine series serves every lane: the
// step of a lane must see the wave a plain launch would show it) but records nothing more, and its state of the moment
// it arrived is what is written back.
template <int IN>
__global__ __launch_bounds__(64) void theta_sequence_rollout_kernel(const AgentArgs a_in, const double* lead, int K,
                                                                    double forward_distance, double* future, int32_t* count,
                                                                    int32_t* diag, int64_t n_agents) {
  const int64_t B = a_in.B;
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool valid = b < B;
  double* const st = a_in.state + (valid ? b : 0);
  double target = 0.0;
  double fin[RIAB_STATE_ROWS];
  if (valid) {
    st[RIAB_S_POS_X * B] = lead[RIAB_S_POS_X * B + b];
    st[RIAB_S_POS_Y * B] = lead[RIAB_S_POS_Y * B + b];
    st[RIAB_S_VEL_X * B] = lead[RIAB_S_VEL_X * B + b];
    st[RIAB_S_VEL_Y * B] = lead[RIAB_S_VEL_Y * B + b];
    st[RIAB_S_ROT_VEL * B] = lead[RIAB_S_ROT_VEL * B + b];
    const double d0 = lead[RIAB_S_DIST * B + b];
    st[RIAB_S_DIST * B] = d0;
    target = d0 + forward_distance;
    future[0 * B + b] = d0;
    future[1 * B + b] = st[RIAB_S_POS_X * B];
    future[2 * B + b] = st[RIAB_S_POS_Y * B];
#pragma unroll
    for (int r = 0; r < RIAB_STATE_ROWS; ++r) fin[r] = st[r * B];
  }
  bool done = !valid || !(fin[RIAB_S_DIST] < target);
  int n = 0;
  AgentArgs a = a_in;
  for (int k = 0; k < K; ++k) {
    if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
    a.step0 = a_in.step0 + (uint64_t)k;
    a.z_in = a_in.z_in ? a_in.z_in + (int64_t)k * 2 * B : nullptr;
    a.z_out = a_in.z_out ? a_in.z_out + (int64_t)k * 2 * B : nullptr;
    agent_step_body<double, IN, false>(a);
    if (!done) {
#pragma unroll
      for (int r = 0; r < RIAB_STATE_ROWS; ++r) fin[r] = st[r * B];
      double* const f = future + (int64_t)(k + 1) * 3 * B + b;
      f[0] = fin[RIAB_S_DIST];
      f[B] = fin[RIAB_S_POS_X];
      f[2 * B] = fin[RIAB_S_POS_Y];
      n = k + 1;
      done = !(fin[RIAB_S_DIST] < target);
    }
  }
  if (!valid) return;
#pragma unroll
  for (int r = 0; r < RIAB_STATE_ROWS; ++r) st[r * B] = fin[r];
  count[b] = n;
  if (!done && diag && b < n_agents) atomicAdd(diag + RIAB_THETA_DIAG_ROLLOUT, 1);
}

__global__ __launch_bounds__(64) void shift_agent_kernel(const double* lead, int64_t B, double shift_m, double* out) {
  RIAB_EXACT_FP
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  // LeadAgent.pos + LeadAgent.head_direction * shift_m (SubAgent.py:476)
  out[b] = lead[RIAB_S_POS_X * B + b] + lead[RIAB_S_HD_X * B + b] * shift_m;
  out[B + b] = lead[RIAB_S_POS_Y * B + b] + lead[RIAB_S_HD_Y * B + b] * shift_m;
}

}  // namespace riab

using namespace riab;

extern "C" int riab_theta_sequence_step(const RiabEnv* env, const double* lead_state, int64_t B, int64_t n_agents, double* ring,
                                        int32_t capacity, int32_t lookback, int64_t n_records, int32_t branch, double phase,
                                        double d_half, double theta_frac, const double* future, const int32_t* count,
                                        int32_t K, double* pos_out, int32_t* diag, riab_stream_t stream) {
  if (!env || !lead_state || !ring || !pos_out || B <= 0 || n_records < 0 || n_agents < 0 || n_agents > B) return RIAB_EINVAL;
  if (B % 4 != 0) return RIAB_EALIGN;
  if (lookback < 1 || capacity < lookback) return RIAB_EINVAL;
  if (branch != RIAB_THETA_NONE && branch != RIAB_THETA_BEHIND && branch != RIAB_THETA_AHEAD) return RIAB_EINVAL;
  if (!(d_half > 0.0) || !(theta_frac > 0.0)) return RIAB_EINVAL;
  if (branch == RIAB_THETA_AHEAD && (!future || !count || K < 1)) return RIAB_EINVAL;
  ThetaStepArgs a;
  a.lead = lead_state;
  a.B = B;
  a.n_agents = n_agents;
  a.ring = ring;
  a.capacity = capacity;
  a.lookback = lookback;
  a.n_before = n_records;
  a.branch = branch;
  a.phase = phase;
  a.d_half = d_half;
  a.theta_frac = theta_frac;
  a.future = future;
  a.count = count;
  a.K = K;
  a.scale = env->scale;
  a.periodic = env->periodic;
  a.out = pos_out;
  a.diag = diag;
  hipLaunchKernelGGL(theta_sequence_step_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

extern "C" int riab_theta_sequence_rollout(const RiabEnv* env, const RiabMotion* motion, const double* lead_state,
                                           double* forward_state, int64_t B, int64_t n_agents, int64_t agent_id0, const double* z_in,
                                           double* z_out, uint64_t seed, uint64_t step0, int32_t K, double forward_distance,
                                           double* future, int32_t* count, int32_t* motion_diag, int32_t* diag,
                                           riab_stream_t stream) {
  if (!lead_state || !future || !count || K < 1 || !(forward_distance > 0.0) || n_agents < 0 || n_agents > B) return RIAB_EINVAL;
  if (B > 0 && B % 4 != 0) return RIAB_EALIGN;
  if (motion && motion->has_drift) return RIAB_EINVAL;
  AgentArgs a;
  const int rc = fill_agent_args(a, env, motion, forward_state, B, agent_id0, nullptr, z_in, z_out, nullptr, seed, step0, 1,
                                 nullptr, motion_diag);
  if (rc) return rc;
  const dim3 grid((unsigned)((B + 63) / 64)), block(64);
  if (z_in) hipLaunchKernelGGL(theta_sequence_rollout_kernel<1>, grid, block, 0, (hipStream_t)stream, a, lead_state, K,
                               forward_distance, future, count, diag, n_agents);
  else hipLaunchKernelGGL(theta_sequence_rollout_kernel<0>, grid, block, 0, (hipStream_t)stream, a, lead_state, K,
                          forward_distance, future, count, diag, n_agents);
  return (int)hipGetLastError();
}

extern "C" int riab_shift_agent_position(const double* lead_state, int64_t B, double shift_m, double* pos_out,
                                         riab_stream_t stream) {
  if (!lead_state || !pos_out || B <= 0) return RIAB_EINVAL;
  if (B % 4 != 0) return RIAB_EALIGN;
  hipLaunchKernelGGL(shift_agent_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, lead_state, B,
                     shift_m, pos_out);
  return (int)hipGetLastError();
}
