// riab_bayes_filter.hip — the Bayesian decoder with a continuity prior, run as a causal forward filter over the windows.
//
// riab_bayes.hip decodes every window from the fitted prior alone.  Here the posterior of window t - 1 is carried to window
// t through a transition that says the animal cannot have moved far (Zhang et al. 1998, two-step reconstruction).  Bins
// j = 0..J-1 lie on a grid (ny, nx), row-major; ok_j: the bin is admissible; g[d], d = -R..R: Gaussian taps that sum to 1.
//
//     q(j')    = p_{t-1}(j') inv_norm_j'          inv_norm_j' = 1 / sum_j G(j - j') ok_j  (0 where j' is not admissible)
//     pred(j)  = (1 - eps) ok_j sum_j' G(j - j') q(j') + eps prior_j         G(r, c) = g[r] g[c], taps off the grid dropped
//     l_t(j)   = loglik_t(j) + log pred(j)       p_t = softmax(l_t)
//
// with pred = prior on the first window of a run, on a window whose restart flag is set, and on the window after one whose
// column did not end with a positive, finite Z ("bad").  loglik_t(j) = sum_c k_c L_cj - tau S_j comes from riab_feedforward
// ([W][Jp][B], -inf in bins that are not admissible); the six outputs per (window, column) are riab_bayes_decode's, row 4
// now being the predictive log likelihood log p(k_t | k_<t).
//
// The scan is sequential in windows and parallel in (bin, column); one window is two launches.
//
//   filter_post_kernel   a workgroup owns 64 columns x one split of the bins, each of its four waves a quarter of the split
//                   (a lane: one column).  Per bin, j ascending: the y-blur of tmp (d ascending, fmaf chain), mask, mix and
//                   log -> log pred, or log prior_j on a fresh column; l = loglik + that is stored to post; the lane keeps
//                   bayes_kernel's running (m, Z, sum p x, sum p y, arg); wave 0 merges the four quarters in the order of
//                   their bins and writes the partial of (split, column).
//   filter_blur_kernel   wave 0 of every workgroup merges the column's S partials in split order (a tie goes to the lower
//                   bin; an empty state subtracts 0, as in bayes_kernel); the workgroups of split 0 write the six outputs
//                   and the bad flag.  Then q = exp2((l - M) log2 e) (inv_norm_j / Z) is formed once per element and staged
//                   in LDS, 64 bins at a time with a halo of R on either side (flat bin index; taps that would leave the grid
//                   row are dropped), and the x-blur of q (d ascending) is written to tmp.
//
// The number of splits is a function of Jp alone and a lane's arithmetic touches its own column only: a column's bits depend
// on neither B, the tile nor its neighbours, and whatever a padding lane holds stays in its column.  No atomics; every word
// of post, tmp, the workspace and out has one owner per launch.  Padding bins J..Jp-1 are written (-inf / 0), never read.
//
// riab_bayes_filter_keep is the same scan with every window's l kept: window w goes through ells[w] where riab_bayes_filter
// goes through post.  The backward smoother (riab_bayes_smooth.hip) reads them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "riab_device.h"   // LOG2E

namespace {

using riab::LOG2E;

constexpr int BF_MAXR = RIAB_BAYES_FILTER_MAX_RADIUS;
constexpr int BF_SEG = 64;    // bins staged in LDS at a time (plus the halo)
constexpr int BF_COLS = 64;   // columns per workgroup: one per lane

struct FilterArgs {
  const float* loglik;      // [Jp][B] of this window
  const float* prior;       // [Jp]
  const float* inv_norm;    // [Jp]
  const float* centres;     // [2][Jp]
  const uint8_t* restart;   // [B] of this window, or null
  float* post;              // [Jp][B]
  float* tmp;               // [Jp][B]
  float* ws;                // [S][5][B] partials, then [B] 32-bit bad flags
  float* out;               // [6][B] of this window
  int64_t B;
  int J, Jp, ny, nx, R, S, chunk;
  int all_fresh;            // the first window of a run: tmp and the bad flags are not read
  float eps, one_minus_eps;
  float taps[BF_MAXR + 1];  // g[0..R]
};

// g[-R..R] into LDS.  The kernel arguments are indexed by constants only (a lane-dependent index into them would have to
// go through a stack copy).
__device__ __forceinline__ void bf_stage_taps(const FilterArgs& a, float* s_g, int tid) {
  const int k = tid < a.R ? a.R - tid : tid - a.R;
  float g = 0.0f;
#pragma unroll
  for (int i = 0; i <= BF_MAXR; ++i)
    if (k == i) g = a.taps[i];
  if (tid <= 2 * a.R) s_g[tid] = g;
}

// (m, Z, sx, sy, arg) += (m_o, Z_o, sx_o, sy_o, arg_o), the state of LATER bins: a tie goes to the lower bin
__device__ __forceinline__ void bf_merge(float& M, float& Z, float& sx, float& sy, int& A, float m_o, float Z_o, float sx_o,
                                         float sy_o, int arg_o) {
  const bool take_o = m_o > M || (m_o == M && arg_o < A);
  const float Mn = take_o ? m_o : M;
  A = take_o ? arg_o : A;
  const float Ms = Mn == -INFINITY ? 0.0f : Mn;   // an empty state subtracts 0
  const float wa = __builtin_amdgcn_exp2f((M - Ms) * LOG2E), wb = __builtin_amdgcn_exp2f((m_o - Ms) * LOG2E);
  Z = __builtin_fmaf(Z_o, wb, Z * wa);
  sx = __builtin_fmaf(sx_o, wb, sx * wa);
  sy = __builtin_fmaf(sy_o, wb, sy * wa);
  M = Mn;
}

__global__ __launch_bounds__(256) void filter_post_kernel(const FilterArgs a) {
  __shared__ float s_g[2 * BF_MAXR + 1];
  __shared__ float s_part[3][5][BF_COLS];   // the states of waves 1..3, merged by wave 0
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  bf_stage_taps(a, s_g, tid);
  __syncthreads();
  const int s = blockIdx.y;   // the range of bins; its four quarters go to the four waves
  const int64_t b = (int64_t)blockIdx.x * BF_COLS + lane;
  const bool live = b < a.B;
  const int64_t bb = live ? b : 0;   // a lane past B reads column 0 and stores nothing
  const int quarter = a.chunk >> 2;
  const int j0 = s * a.chunk + wave * quarter;
  const int j1 = j0 + quarter < a.Jp ? j0 + quarter : a.Jp;
  const float neg_inf = -INFINITY;
  const uint32_t* bad = reinterpret_cast<const uint32_t*>(a.ws + (int64_t)5 * a.S * a.B);
  bool fresh = true;
  if (!a.all_fresh) fresh = (a.restart && a.restart[bb] != 0) || bad[bb] != 0u;

  float m = neg_inf, Z = 0.0f, sx = 0.0f, sy = 0.0f;
  int arg = j0;
  int r = j0 / a.nx, c = j0 - r * a.nx;
  for (int j = j0; j < j1; ++j) {
    float* const dst = a.post + (int64_t)j * a.B + bb;
    if (j >= a.J) {   // padding bins: written, never read
      if (live) *dst = neg_inf;
      continue;
    }
    const float pr = a.prior[j];
    const float lprior = logf(pr);
    float lp = lprior;
    if (!a.all_fresh) {
      const int dlo = r < a.R ? -r : -a.R;
      const int dhi = a.ny - 1 - r < a.R ? a.ny - 1 - r : a.R;
      const float* src = a.tmp + ((int64_t)j + (int64_t)dlo * a.nx) * a.B + bb;
      const int64_t step = (int64_t)a.nx * a.B;
      float acc = 0.0f;
      for (int d = dlo; d <= dhi; ++d, src += step) acc = __builtin_fmaf(s_g[d + a.R], *src, acc);
      const float pred = a.inv_norm[j] > 0.0f ? __builtin_fmaf(a.one_minus_eps, acc, a.eps * pr) : 0.0f;
      lp = fresh ? lprior : logf(pred);
    }
    const float v = a.loglik[(int64_t)j * a.B + bb] + lp;
    if (live) *dst = v;
    if (v > m) {   // strictly greater, j ascending: the lowest index wins a tie; NaN never wins
      const float sc = __builtin_amdgcn_exp2f((m - v) * LOG2E);
      Z *= sc;
      sx *= sc;
      sy *= sc;
      m = v;
      arg = j;
    }
    const float ms = m == neg_inf ? 0.0f : m;   // an empty state subtracts 0: -inf - -inf is never formed
    const float p = __builtin_amdgcn_exp2f((v - ms) * LOG2E);
    Z += p;
    sx = __builtin_fmaf(p, a.centres[j], sx);
    sy = __builtin_fmaf(p, a.centres[(int64_t)a.Jp + j], sy);
    if (++c == a.nx) {
      c = 0;
      ++r;
    }
  }
  if (wave > 0) {
    s_part[wave - 1][0][lane] = m;
    s_part[wave - 1][1][lane] = Z;
    s_part[wave - 1][2][lane] = sx;
    s_part[wave - 1][3][lane] = sy;
    s_part[wave - 1][4][lane] = __int_as_float(arg);
  }
  __syncthreads();
  if (wave > 0 || !live) return;
#pragma unroll
  for (int w = 0; w < 3; ++w)   // the quarters in the order of their bins
    bf_merge(m, Z, sx, sy, arg, s_part[w][0][lane], s_part[w][1][lane], s_part[w][2][lane], s_part[w][3][lane],
             __float_as_int(s_part[w][4][lane]));
  float* w = a.ws + (int64_t)s * 5 * a.B + b;
  w[0] = m;
  w[a.B] = Z;
  w[2 * a.B] = sx;
  w[3 * a.B] = sy;
  reinterpret_cast<int*>(w)[4 * a.B] = arg;
}

__global__ __launch_bounds__(256) void filter_blur_kernel(const FilterArgs a) {
  __shared__ float s_q[BF_SEG + 2 * BF_MAXR][BF_COLS];
  __shared__ float s_g[2 * BF_MAXR + 1];
  __shared__ float s_m[BF_COLS], s_rz[BF_COLS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  bf_stage_taps(a, s_g, tid);
  const int64_t b = (int64_t)blockIdx.x * BF_COLS + lane;
  const bool live = b < a.B;
  const int64_t bb = live ? b : 0;   // a lane past B reads column 0 and stores nothing
  const float neg_inf = -INFINITY;
  if (wave == 0) {
    const float* w = a.ws + bb;
    float M = w[0], Z = w[a.B], sx = w[2 * a.B], sy = w[3 * a.B];
    int A = reinterpret_cast<const int*>(w)[4 * a.B];
#pragma unroll 4
    for (int s = 1; s < a.S; ++s) {
      w += 5 * a.B;
      bf_merge(M, Z, sx, sy, A, w[0], w[a.B], w[2 * a.B], w[3 * a.B], reinterpret_cast<const int*>(w)[4 * a.B]);
    }
    A = A < a.J ? A : a.J - 1;
    const bool ok = Z > 0.0f && Z < INFINITY;   // (false for NaN)
    const float nan = __uint_as_float(0x7fc00000u);
    s_m[lane] = M;
    s_rz[lane] = ok ? 1.0f / Z : nan;
    if (blockIdx.y == 0 && live) {
      float* o = a.out + b;
      o[0] = ok ? sx / Z : nan;
      o[a.B] = ok ? sy / Z : nan;
      o[2 * a.B] = ok ? a.centres[A] : nan;
      o[3 * a.B] = ok ? a.centres[(int64_t)a.Jp + A] : nan;
      o[4 * a.B] = ok ? M + logf(Z) : nan;
      o[5 * a.B] = ok ? 1.0f / Z : nan;
      reinterpret_cast<uint32_t*>(a.ws + (int64_t)5 * a.S * a.B)[b] = ok ? 0u : 1u;
    }
  }
  __syncthreads();
  const float M = s_m[lane], rZ = s_rz[lane];
  const int B0 = blockIdx.y * 4 * a.chunk;
  const int B1 = B0 + 4 * a.chunk < a.Jp ? B0 + 4 * a.chunk : a.Jp;
  for (int t0 = B0; t0 < B1; t0 += BF_SEG) {
    const int n = B1 - t0 < BF_SEG ? B1 - t0 : BF_SEG;
    for (int i0 = wave * 4; i0 < n + 2 * a.R; i0 += 16) {   // four rows a turn: their loads are in flight together
      float l[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {   // (rows outside the bins, or past the stage, read a bin inside and are not used)
        const int j = t0 - a.R + i0 + u;
        const int jc = j < 0 ? 0 : (j < a.J ? j : a.J - 1);
        l[u] = a.post[(int64_t)jc * a.B + bb];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u, j = t0 - a.R + i;
        if (i < n + 2 * a.R) {
          const bool in = j >= 0 && j < a.J;
          const float q = __builtin_amdgcn_exp2f((l[u] - M) * LOG2E) * (a.inv_norm[in ? j : 0] * rZ);
          s_q[i][lane] = in ? q : 0.0f;
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
        for (int d = dlo; d <= dhi; ++d) acc = __builtin_fmaf(s_g[d + a.R], s_q[i + a.R + d][lane], acc);
      }
      if (live) a.tmp[(int64_t)j * a.B + b] = acc;
    }
    __syncthreads();
  }
}

// The checks and the launches of both exports.  `ells` null: every window's l goes through post; else window w's goes through
// ells + w Jp B (written by filter_post_kernel, re-read by filter_blur_kernel: the same two kernels on another address).
static int filter_run(const float* loglik, int64_t W, int32_t J, int32_t Jp, int32_t ny, int32_t nx, int64_t B, int32_t radius,
                      const float* taps, float mixing, const float* prior, const float* inv_norm, const float* centres,
                      const uint8_t* restart, int32_t first, float* post, float* ells, float* tmp, float* workspace, float* out,
                      riab_stream_t stream) {
  if (!loglik || !taps || !prior || !inv_norm || !centres || !post || !tmp || !workspace || !out) return RIAB_EINVAL;
  if (W < 0 || J < 1 || Jp < J || ny < 1 || nx < 1 || B <= 0) return RIAB_EINVAL;
  if ((int64_t)ny * nx != J) return RIAB_EINVAL;
  if (radius < 1 || radius > RIAB_BAYES_FILTER_MAX_RADIUS) return RIAB_EINVAL;
  if (!(mixing > 0.0f && mixing <= 1.0f)) return RIAB_EINVAL;
  for (int i = 0; i <= radius; ++i)
    if (!(taps[i] >= 0.0f && taps[i] <= 1.0f)) return RIAB_EINVAL;
  if (J > RIAB_RATEMAP_MAX_BINS) return RIAB_EUNSUPPORTED;
  if ((B & 3) || (Jp & 31)) return RIAB_EALIGN;
  if (((uintptr_t)loglik | (uintptr_t)prior | (uintptr_t)inv_norm | (uintptr_t)centres | (uintptr_t)post | (uintptr_t)tmp |
       (uintptr_t)workspace | (uintptr_t)out) & 15)
    return RIAB_EALIGN;
  const int64_t tiles = (B + BF_COLS - 1) / BF_COLS;
  if (tiles > 0x7fffffffLL || W > 65535) return RIAB_ETOOBIG;
  if (W == 0) return RIAB_OK;
  FilterArgs a = {};
  a.prior = prior;
  a.inv_norm = inv_norm;
  a.centres = centres;
  a.post = post;
  a.tmp = tmp;
  a.ws = workspace;
  a.B = B;
  a.J = J;
  a.Jp = Jp;
  a.ny = ny;
  a.nx = nx;
  a.R = radius;
  a.S = RIAB_BAYES_FILTER_SPLITS(Jp);
  a.chunk = Jp <= 512 ? 32 : 128;
  a.eps = mixing;
  a.one_minus_eps = 1.0f - mixing;
  for (int i = 0; i <= radius; ++i) a.taps[i] = taps[i];
  const dim3 grid_post((unsigned)tiles, (unsigned)a.S), grid_blur((unsigned)tiles, (unsigned)((a.S + 3) / 4));
  for (int64_t w = 0; w < W; ++w) {
    a.loglik = loglik + w * Jp * B;
    if (ells) a.post = ells + w * Jp * B;
    a.restart = restart ? restart + w * B : nullptr;
    a.out = out + w * RIAB_BAYES_OUT_ROWS * B;
    a.all_fresh = (first && w == 0) ? 1 : 0;
    hipLaunchKernelGGL(filter_post_kernel, grid_post, dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(filter_blur_kernel, grid_blur, dim3(256), 0, (hipStream_t)stream, a);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return RIAB_OK;
}

}  // namespace

extern "C" int riab_bayes_filter(const float* loglik, int64_t W, int32_t J, int32_t Jp, int32_t ny, int32_t nx, int64_t B,
                                 int32_t radius, const float* taps, float mixing, const float* prior, const float* inv_norm,
                                 const float* centres, const uint8_t* restart, int32_t first, float* post, float* tmp,
                                 float* workspace, float* out, riab_stream_t stream) {
  return filter_run(loglik, W, J, Jp, ny, nx, B, radius, taps, mixing, prior, inv_norm, centres, restart, first, post, nullptr,
                    tmp, workspace, out, stream);
}

extern "C" int riab_bayes_filter_keep(const float* loglik, int64_t W, int32_t J, int32_t Jp, int32_t ny, int32_t nx, int64_t B,
                                      int32_t radius, const float* taps, float mixing, const float* prior,
                                      const float* inv_norm, const float* centres, const uint8_t* restart, int32_t first,
                                      float* ells, float* tmp, float* workspace, float* out, riab_stream_t stream) {
  // (ells stands in post's place in the checks: null is RIAB_EINVAL, a misaligned one RIAB_EALIGN)
  return filter_run(loglik, W, J, Jp, ny, nx, B, radius, taps, mixing, prior, inv_norm, centres, restart, first, ells, ells, tmp,
                    workspace, out, stream);
}
