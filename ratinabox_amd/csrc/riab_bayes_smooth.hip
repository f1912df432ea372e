// riab_bayes_smooth.hip — the backward pass behind the forward filter of riab_bayes_filter.hip: the smoothed posterior
// p(x_t | k_1..k_T) of every window of a recorded run.
//
// Notation of riab_bayes_filter.hip: bins j on the grid (ny, nx), ok_j, prior_j, taps g[-R..R], inv_norm, eps = mixing.  The
// forward filter (riab_bayes_filter_keep) left l_t [Jp][B] of every window and its six outputs; ev_t is its row 4,
// log p(k_t | k_<t).  With beta_{T-1} = 1 and t descending,
//
//     u_{t+1}(j) = exp(loglik_{t+1}(j) - ev_{t+1}) beta_{t+1}(j)                       0 where j is not admissible
//     c_t        = sum_j prior_j u_{t+1}(j)
//     beta_t(j') = (1 - eps) inv_norm_j' sum_j G(j - j') u_{t+1}(j) + eps c_t ok_j'    taps off the grid dropped
//     gamma_t(j) = p_t(j) beta_t(j) / sum_i p_t(i) beta_t(i)                           p_t(j) = exp(l_t(j) - ev_t)
//
// In this scaling sum_i p_t beta_t = 1 in exact arithmetic and beta <= 1 / (eps min prior): float32 needs no rescaling per
// window.  The chain is CUT at window t (beta_t = 1, the six outputs are the filter's, copied) when t is the run's last
// window, when window t + 1 has its restart flag set or came out as NaN, or when window t itself came out as NaN.
//
// The scan is sequential in windows, last to first, and parallel in (bin, column); one window is two launches, in the
// filter's shapes (a lane is a column, four waves share a range of bins, RIAB_BAYES_FILTER_SPLITS(Jp) ranges).
//
//   smooth_gamma_kernel  (window t) a workgroup owns 64 columns x one range of the bins.  c_t: the partials of the u stage,
//                   added in their order.  Per bin, j ascending: the y-blur of tmp (d ascending, fmaf chain), beta_t (1 on
//                   a cut column) stored to beta; gamma's unnormalised value exp2((l_t - ev_t) log2 e) beta_t; the lane keeps
//                   the running (max, arg, sum gamma, sum gamma x, sum gamma y); wave 0 merges the four quarters in the
//                   order of their bins and writes the partial of (range, column).
//   smooth_u_kernel      (window t, after it) the workgroups of range 0 merge the column's partials in range order (strict >:
//                   the lowest bin wins a tie, NaN never wins), write the six outputs of window t and the cut flag the
//                   window to the LEFT will read (restart flag of t, or ev_t is NaN).  Then u_t is formed once per staged
//                   element in LDS, 64 bins at a time with a halo of R either side, the x-blur of u_t (d ascending) is
//                   written to tmp, and the workgroup's share of sum_j prior_j u_t(j) to the workspace.
//
// So beta, tmp and the workspace after a call hold what the window to the left of the call needs, and a run may be given in
// several calls, rightmost first.  A lane's arithmetic touches its own column only and the split is a function of Jp alone:
// a column's bits depend on neither B, its neighbours nor how the windows are batched into calls.  No atomics; every word
// of beta, tmp, the workspace and out has one owner per launch.  Padding bins J..Jp-1 of beta / tmp are written (0), never
// read; a lane past B reads column 0 and stores nothing.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "riab_device.h"   // LOG2E

namespace {

using riab::LOG2E;

constexpr int BS_MAXR = RIAB_BAYES_FILTER_MAX_RADIUS;
constexpr int BS_SEG = 64;    // bins staged in LDS at a time (plus the halo)
constexpr int BS_COLS = 64;   // columns per workgroup: one per lane

struct SmoothArgs {
  const float* loglik;      // [Jp][B] of this window
  const float* ell;         // [Jp][B] of this window: the filter's l
  const float* filt;        // [6][B] of this window: the filter's outputs
  const float* prior;       // [Jp]
  const float* inv_norm;    // [Jp]
  const float* centres;     // [2][Jp]
  const uint8_t* restart;   // [B] of this window, or null
  float* beta;              // [Jp][B]
  float* tmp;               // [Jp][B]
  float* ws;                // [S][5][B] partials of gamma, [SU][B] partials of c, then [B] 32-bit cut flags
  float* out;               // [6][B] of this window
  int64_t B;
  int J, Jp, ny, nx, R, S, SU, chunk;
  int all_cut;              // the last window of a run: tmp, the partials of c and the cut flags are not read
  float eps, one_minus_eps;
  float taps[BS_MAXR + 1];  // g[0..R]
};

// g[-R..R] into LDS.  The kernel arguments are indexed by constants only (a lane-dependent index into them would have to
// go through a stack copy).
__device__ __forceinline__ void bs_stage_taps(const SmoothArgs& a, float* s_g, int tid) {
  const int k = tid < a.R ? a.R - tid : tid - a.R;
  float g = 0.0f;
#pragma unroll
  for (int i = 0; i <= BS_MAXR; ++i)
    if (k == i) g = a.taps[i];
  if (tid <= 2 * a.R) s_g[tid] = g;
}

__device__ __forceinline__ const uint32_t* bs_flags(const SmoothArgs& a) {
  return reinterpret_cast<const uint32_t*>(a.ws + (int64_t)(5 * a.S + a.SU) * a.B);
}

// (mx, Z, sx, sy, arg) += (mx_o, ...), the state of LATER bins: plain sums, and a tie of the maxima stays with the lower bin
__device__ __forceinline__ void bs_merge(float& mx, float& Z, float& sx, float& sy, int& A, float mx_o, float Z_o, float sx_o,
                                         float sy_o, int arg_o) {
  const bool take_o = mx_o > mx;
  mx = take_o ? mx_o : mx;
  A = take_o ? arg_o : A;
  Z += Z_o;
  sx += sx_o;
  sy += sy_o;
}

__global__ __launch_bounds__(256) void smooth_gamma_kernel(const SmoothArgs a) {
  __shared__ float s_g[2 * BS_MAXR + 1];
  __shared__ float s_part[3][5][BS_COLS];   // the states of waves 1..3, merged by wave 0
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  bs_stage_taps(a, s_g, tid);
  __syncthreads();
  const int s = blockIdx.y;   // the range of bins; its four quarters go to the four waves
  const int64_t b = (int64_t)blockIdx.x * BS_COLS + lane;
  const bool live = b < a.B;
  const int64_t bb = live ? b : 0;   // a lane past B reads column 0 and stores nothing
  const int quarter = a.chunk >> 2;
  const int j0 = s * a.chunk + wave * quarter;
  const int j1 = j0 + quarter < a.Jp ? j0 + quarter : a.Jp;
  const float ev = a.filt[4 * a.B + bb];
  bool cut = true;
  float c = 0.0f;
  if (!a.all_cut) {
    cut = bs_flags(a)[bb] != 0u || !(ev == ev);
    const float* cp = a.ws + (int64_t)5 * a.S * a.B + bb;
    c = cp[0];
    for (int i = 1; i < a.SU; ++i) c += cp[(int64_t)i * a.B];   // in the order of their bins
  }
  const float eps_c = a.eps * c;

  float mx = -INFINITY, Z = 0.0f, sx = 0.0f, sy = 0.0f;
  int arg = j0;
  int r = j0 / a.nx, col = j0 - r * a.nx;
  for (int j = j0; j < j1; ++j) {
    float* const dst = a.beta + (int64_t)j * a.B + bb;
    if (j >= a.J) {   // padding bins: written, never read
      if (live) *dst = 0.0f;
      continue;
    }
    float bt = 1.0f;
    if (!a.all_cut) {
      const int dlo = r < a.R ? -r : -a.R;
      const int dhi = a.ny - 1 - r < a.R ? a.ny - 1 - r : a.R;
      const float* src = a.tmp + ((int64_t)j + (int64_t)dlo * a.nx) * a.B + bb;
      const int64_t step = (int64_t)a.nx * a.B;
      float acc = 0.0f;
      for (int d = dlo; d <= dhi; ++d, src += step) acc = __builtin_fmaf(s_g[d + a.R], *src, acc);
      const float inv = a.inv_norm[j];
      const float carried = inv > 0.0f ? __builtin_fmaf(a.one_minus_eps * inv, acc, eps_c) : 0.0f;
      bt = cut ? 1.0f : carried;   // a select: whatever a cut column's tmp holds stays out
    }
    if (live) *dst = bt;
    const float gam = __builtin_amdgcn_exp2f((a.ell[(int64_t)j * a.B + bb] - ev) * LOG2E) * bt;
    if (gam > mx) {   // strictly greater, j ascending: the lowest index wins a tie; NaN never wins
      mx = gam;
      arg = j;
    }
    Z += gam;
    sx = __builtin_fmaf(gam, a.centres[j], sx);
    sy = __builtin_fmaf(gam, a.centres[(int64_t)a.Jp + j], sy);
    if (++col == a.nx) {
      col = 0;
      ++r;
    }
  }
  if (wave > 0) {
    s_part[wave - 1][0][lane] = mx;
    s_part[wave - 1][1][lane] = Z;
    s_part[wave - 1][2][lane] = sx;
    s_part[wave - 1][3][lane] = sy;
    s_part[wave - 1][4][lane] = __int_as_float(arg);
  }
  __syncthreads();
  if (wave > 0 || !live) return;
#pragma unroll
  for (int w = 0; w < 3; ++w)   // the quarters in the order of their bins
    bs_merge(mx, Z, sx, sy, arg, s_part[w][0][lane], s_part[w][1][lane], s_part[w][2][lane], s_part[w][3][lane],
             __float_as_int(s_part[w][4][lane]));
  float* w = a.ws + (int64_t)s * 5 * a.B + b;
  w[0] = mx;
  w[a.B] = Z;
  w[2 * a.B] = sx;
  w[3 * a.B] = sy;
  reinterpret_cast<int*>(w)[4 * a.B] = arg;
}

__global__ __launch_bounds__(256) void smooth_u_kernel(const SmoothArgs a) {
  __shared__ float s_u[BS_SEG + 2 * BS_MAXR][BS_COLS];
  __shared__ float s_g[2 * BS_MAXR + 1];
  __shared__ float s_ev[BS_COLS];
  __shared__ float s_c[3][BS_COLS];   // the shares of waves 1..3, added by wave 0
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  bs_stage_taps(a, s_g, tid);
  const int64_t b = (int64_t)blockIdx.x * BS_COLS + lane;
  const bool live = b < a.B;
  const int64_t bb = live ? b : 0;   // a lane past B reads column 0 and stores nothing
  if (wave == 0) {
    const float ev = a.filt[4 * a.B + bb];
    s_ev[lane] = ev;
    if (blockIdx.y == 0 && live) {   // the outputs of this window, and the flag for the window to its left
      const float* w = a.ws + b;
      float mx = w[0], Z = w[a.B], sx = w[2 * a.B], sy = w[3 * a.B];
      int A = reinterpret_cast<const int*>(w)[4 * a.B];
#pragma unroll 4
      for (int s = 1; s < a.S; ++s) {
        w += 5 * a.B;
        bs_merge(mx, Z, sx, sy, A, w[0], w[a.B], w[2 * a.B], w[3 * a.B], reinterpret_cast<const int*>(w)[4 * a.B]);
      }
      A = A < a.J ? A : a.J - 1;
      uint32_t* const flag = reinterpret_cast<uint32_t*>(a.ws + (int64_t)(5 * a.S + a.SU) * a.B) + b;
      const bool bad = !(ev == ev);
      const bool cut = a.all_cut || *flag != 0u || bad;
      const bool ok = Z > 0.0f && Z < INFINITY;   // (false for NaN)
      const float nan = __uint_as_float(0x7fc00000u);
      const float* f = a.filt + b;
      float* o = a.out + b;
      o[0] = cut ? f[0] : (ok ? sx / Z : nan);
      o[a.B] = cut ? f[a.B] : (ok ? sy / Z : nan);
      o[2 * a.B] = cut ? f[2 * a.B] : (ok ? a.centres[A] : nan);
      o[3 * a.B] = cut ? f[3 * a.B] : (ok ? a.centres[(int64_t)a.Jp + A] : nan);
      o[4 * a.B] = ev;
      o[5 * a.B] = cut ? f[5 * a.B] : (ok ? mx / Z : nan);
      *flag = ((a.restart && a.restart[b] != 0) || bad) ? 1u : 0u;
    }
  }
  __syncthreads();
  const float ev = s_ev[lane];
  float pc = 0.0f;
  const int B0 = blockIdx.y * 4 * a.chunk;
  const int B1 = B0 + 4 * a.chunk < a.Jp ? B0 + 4 * a.chunk : a.Jp;
  for (int t0 = B0; t0 < B1; t0 += BS_SEG) {
    const int n = B1 - t0 < BS_SEG ? B1 - t0 : BS_SEG;
    for (int i0 = wave * 4; i0 < n + 2 * a.R; i0 += 16) {   // four rows a turn: their loads are in flight together
      float l[4], bt[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {   // (rows outside the bins, or past the stage, read a bin inside and are not used)
        const int j = t0 - a.R + i0 + u;
        const int jc = j < 0 ? 0 : (j < a.J ? j : a.J - 1);
        l[u] = a.loglik[(int64_t)jc * a.B + bb];
        bt[u] = a.beta[(int64_t)jc * a.B + bb];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u, j = t0 - a.R + i;
        if (i < n + 2 * a.R) {
          const bool in = j >= 0 && j < a.J && a.inv_norm[j >= 0 && j < a.J ? j : 0] > 0.0f;
          const float v = __builtin_amdgcn_exp2f((l[u] - ev) * LOG2E) * bt[u];
          s_u[i][lane] = in ? v : 0.0f;
        }
      }
    }
    __syncthreads();
    for (int i = wave; i < n; i += 4) {
      const int j = t0 + i;
      float acc = 0.0f;
      if (j < a.J) {
        const int c = j % a.nx;
        const int dlo = c < a.R ? -c : -a.R;
        const int dhi = a.nx - 1 - c < a.R ? a.nx - 1 - c : a.R;
        for (int d = dlo; d <= dhi; ++d) acc = __builtin_fmaf(s_g[d + a.R], s_u[i + a.R + d][lane], acc);
        pc = __builtin_fmaf(a.prior[j], s_u[i + a.R][lane], pc);
      }
      if (live) a.tmp[(int64_t)j * a.B + b] = acc;
    }
    __syncthreads();
  }
  if (wave > 0) s_c[wave - 1][lane] = pc;
  __syncthreads();
  if (wave > 0 || !live) return;
  pc += s_c[0][lane];
  pc += s_c[1][lane];
  pc += s_c[2][lane];
  a.ws[(int64_t)(5 * a.S + blockIdx.y) * a.B + b] = pc;
}

}  // namespace

extern "C" int riab_bayes_smooth(const float* loglik, const float* ells, const float* filtered, int64_t W, int32_t J, int32_t Jp,
                                 int32_t ny, int32_t nx, int64_t B, int32_t radius, const float* taps, float mixing,
                                 const float* prior, const float* inv_norm, const float* centres, const uint8_t* restart,
                                 int32_t last, float* beta, float* tmp, float* workspace, float* out, riab_stream_t stream) {
  if (!loglik || !ells || !filtered || !taps || !prior || !inv_norm || !centres || !beta || !tmp || !workspace || !out)
    return RIAB_EINVAL;
  if (W < 0 || J < 1 || Jp < J || ny < 1 || nx < 1 || B <= 0) return RIAB_EINVAL;
  if ((int64_t)ny * nx != J) return RIAB_EINVAL;
  if (radius < 1 || radius > RIAB_BAYES_FILTER_MAX_RADIUS) return RIAB_EINVAL;
  if (!(mixing > 0.0f && mixing <= 1.0f)) return RIAB_EINVAL;
  for (int i = 0; i <= radius; ++i)
    if (!(taps[i] >= 0.0f && taps[i] <= 1.0f)) return RIAB_EINVAL;
  if (J > RIAB_RATEMAP_MAX_BINS) return RIAB_EUNSUPPORTED;
  if ((B & 3) || (Jp & 31)) return RIAB_EALIGN;
  if (((uintptr_t)loglik | (uintptr_t)ells | (uintptr_t)filtered | (uintptr_t)prior | (uintptr_t)inv_norm | (uintptr_t)centres |
       (uintptr_t)beta | (uintptr_t)tmp | (uintptr_t)workspace | (uintptr_t)out) & 15)
    return RIAB_EALIGN;
  const int64_t tiles = (B + BS_COLS - 1) / BS_COLS;
  if (tiles > 0x7fffffffLL || W > 65535) return RIAB_ETOOBIG;
  if (W == 0) return RIAB_OK;
  SmoothArgs a = {};
  a.prior = prior;
  a.inv_norm = inv_norm;
  a.centres = centres;
  a.beta = beta;
  a.tmp = tmp;
  a.ws = workspace;
  a.B = B;
  a.J = J;
  a.Jp = Jp;
  a.ny = ny;
  a.nx = nx;
  a.R = radius;
  a.S = RIAB_BAYES_FILTER_SPLITS(Jp);
  a.SU = (a.S + 3) / 4;
  a.chunk = Jp <= 512 ? 32 : 128;
  a.eps = mixing;
  a.one_minus_eps = 1.0f - mixing;
  for (int i = 0; i <= radius; ++i) a.taps[i] = taps[i];
  const dim3 grid_gamma((unsigned)tiles, (unsigned)a.S), grid_u((unsigned)tiles, (unsigned)a.SU);
  for (int64_t w = W - 1; w >= 0; --w) {
    a.loglik = loglik + w * Jp * B;
    a.ell = ells + w * Jp * B;
    a.filt = filtered + w * RIAB_BAYES_OUT_ROWS * B;
    a.restart = restart ? restart + w * B : nullptr;
    a.out = out + w * RIAB_BAYES_OUT_ROWS * B;
    a.all_cut = (last && w == W - 1) ? 1 : 0;
    hipLaunchKernelGGL(smooth_gamma_kernel, grid_gamma, dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(smooth_u_kernel, grid_u, dim3(256), 0, (hipStream_t)stream, a);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return RIAB_OK;
}
