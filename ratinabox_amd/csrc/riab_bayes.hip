// riab_bayes.hip — Poisson maximum-likelihood ("Bayesian") decoding of position from spike counts, in one fused kernel.
//
// Cells c = 1..n with tuning curves f_cj >= 0 (Hz) over bins j = 1..J with centres x_j; a window of duration tau holds
// k_c spikes of cell c (or tau * rate_c).  With L_cj = log max(f_cj, floor) and bias_j = log prior_j - tau sum_c max(f_cj,
// floor) (ratinabox_amd/_bayes_decoder.py builds both), the log posterior of bin j is
//
//     l_j = sum_c k_c L_cj + bias_j                       (bias_j = -inf: the bin is not admissible)
//
// and a (window, agent) sample is reduced to six numbers: the posterior mean sum_j softmax(l)_j x_j, the centre of the
// lowest-indexed bin among the maxima (MAP), logsumexp_j l_j and softmax(l) at the MAP bin.  The sum over cells is a GEMM
// [J bins] x [n cells] x [samples], which runs on the streamed core of csrc/riab_mfma_slab.h (layouts, bounds and barriers are
// stated there), as gp_kernel's does: the table of log rates is operand A, a running softmax takes the place of the RBF sum.
// The [samples] x [J] matrix lives in accumulator registers only.
//
//   bayes_kernel<MT, COUNTS>   grid (position tiles of 128 x windows), 4 waves.  The bins are walked in blocks of 32 MT; for
//                   each block the whole K (every population) is contracted into MT accumulator tiles.  The inputs are uint8
//                   counts (COUNTS: widened to fp32 by the fetch; small integers are exact) or fp32 rates multiplied by
//                   `scale` (by the fetch too).  The stash's select zeroes the table's padding bins J..Jp-1 whatever they
//                   hold.  The epilogue adds bias_j and folds the block into the lane's running state.
//
// Arithmetic of one position, in order.  dot_j = the k-ordered fmaf chain of the MFMA; l_j = dot_j + bias_j.  Each half-wave
// (rows 4h..4h+3 of every group of 8 bins) keeps (m, Z, sx, sy, arg) and takes its bins four at a time, j ascending: the
// new maximum is found by strict > in the order of j (so the lowest index wins a tie); if it rose, Z, sx and sy are
// multiplied by exp2((m_old - m_new) log2 e) once; then p = exp2((l_j - m) log2 e) (v_exp_f32), Z += p, sx = fma(p, x_j, sx),
// sy likewise.  While a state has seen only inadmissible bins m stays -inf ("empty") and 0 is subtracted in its place: no
// -inf - -inf is ever formed.  The two halves are merged once at the end, low half first (a tie between them goes to the
// lower bin).  Nothing of this depends on T, B, the tile or the lane, nor on MT (a block of 32 MT bins is walked in the
// order of j), so a window decoded alone has the bits it has inside a many-window call.  No atomics, no workspace.
//
// Columns are independent: whatever a padding lane holds stays in its own column of the MFMA and of the epilogue.  A
// column whose Z does not end positive and finite — no admissible bin, or a NaN rate — is written as six NaNs.
//
//   window_counts_kernel   the bandwidth side: spike rows of a history piece added into the uint8 counts of the windows
//                   they belong to, four lanes per thread, each byte on its own (a padding lane that holds 255 wraps
//                   inside its byte).  Every output byte has one owner; calls of one decode are ordered on the stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "riab_device.h"   // LOG2E
#include "riab_mfma_slab.h"

namespace {

using namespace riab;

struct BayesArgs {
  const void* rows[RIAB_FF_MAX_INPUTS];    // [T][n_in][B]: uint8 counts or fp32 rates
  const float* wt[RIAB_FF_MAX_INPUTS];     // [n_in][Jp]: log max(f, floor) of the population
  int n_in[RIAB_FF_MAX_INPUTS];
  int n_layers;
  const float* bias;      // [Jp]
  const float* centres;   // [2][Jp]
  int J, Jp;
  int64_t B;
  int tiles;              // position tiles per window
  float scale;            // rates only
  float* out;             // [T][6][B]
};

// bayes_kernel's fetch of uint8 counts, widened to fp32 (small integers are exact): fetch_f32's rows and clamps, 4 bytes
// where that reads 16.
__device__ __forceinline__ Slab by_fetch_u8(const uint8_t* src, int64_t ld, int col, int K, int kbase) {
  Slab f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int k = kbase + 2 * s;
    const int kc = k < K ? k : K - 1;
    const uint32_t w = *reinterpret_cast<const uint32_t*>(src + (int64_t)kc * ld + col);
    f.v[s] = v4f{(float)(w & 255u), (float)((w >> 8) & 255u), (float)((w >> 16) & 255u), (float)(w >> 24)};
  }
  return f;
}

// The running softmax of one half-wave's bins of one column.
struct BayesState {
  float m, Z, sx, sy;
  int arg;
};

// 3 waves per SIMD keep 3 workgroups on a CU, as gp_kernel has them.  The 128-bin form wants 172-174 registers where 168
// are to be had: held to (3, 3) its rates form put two of them in scratch; asked for 2..3 waves the compiler finds 168
// without scratch (no kernel of the library but the known ones may have a stack frame: tests/test_handover_isa.py).
// On the shared core the rates form comes out at 165 either way; the range stays, since 3 registers of slack is what a
// change of statement order moves.
template <int MT, bool COUNTS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((MT == 4 && !COUNTS) ? 2 : 3, 3)))
void bayes_kernel(const BayesArgs a) {
  __shared__ __align__(16) SlabTiles<MT> lds;                     // table slab (A) and input slab
  __shared__ __align__(16) float s_bias[MT * 32];                 // bias of the bin block (bins >= J: -inf)
  __shared__ __align__(16) float s_cx[MT * 32];                   // centres of the bin block
  __shared__ __align__(16) float s_cy[MT * 32];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = blockIdx.x / a.tiles;
  const int64_t b0 = (int64_t)(blockIdx.x - t * a.tiles) * NB;

  const SlabRole<MT> role(lds, tid, wave);
  const Frag<MT> fr(lane, wave);
  const bool is_b = role.is_b;
  const int c4 = role.c4;
  const bool b_ok = b0 + c4 < a.B;                       // (B % 4 == 0: a quad is wholly inside or outside)
  const int kh = fr.kh, j = fr.j;
  const float neg_inf = -INFINITY;

  BayesState st = {neg_inf, 0.0f, 0.0f, 0.0f, 0};
  int buf = 0;
  for (int m0 = 0; m0 < a.Jp; m0 += MT * 32) {   // bin blocks
    // the table's padding bins J..Jp-1 are zeroed whatever they hold: their products must not reach the softmax as NaN
    const SlabMask mask = {is_b ? b_ok : role.a_quad_ok(m0, a.Jp), is_b ? 4 : a.J - (m0 + c4)};
    // the block's and the tile's offsets are wave-uniform and go into the base pointer: the lane keeps one 32-bit column
    const int col = mask.col_ok ? c4 : 0;
    v16f acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) zero_acc(acc[i]);
    for (int l = 0; l < a.n_layers; ++l) {
      const int K = a.n_in[l];
      __syncthreads();  // the slab and the epilogue tables before this have been consumed
      if (l == 0 && tid < MT * 32) {
        const bool in = m0 + tid < a.J;
        s_bias[tid] = in ? a.bias[m0 + tid] : neg_inf;
        s_cx[tid] = in ? a.centres[m0 + tid] : 0.0f;
        s_cy[tid] = in ? a.centres[(int64_t)a.Jp + m0 + tid] : 0.0f;
      }
      contract_population(lds, role, fr, buf, K, mask, acc, [&](int kbase) {
        if (!is_b) return fetch_f32(a.wt[l] + m0, a.Jp, col, K, kbase);
        if (COUNTS) return by_fetch_u8(static_cast<const uint8_t*>(a.rows[l]) + (int64_t)t * K * a.B + b0, a.B, col, K, kbase);
        Slab f = fetch_f32(static_cast<const float*>(a.rows[l]) + (int64_t)t * K * a.B + b0, a.B, col, K, kbase);
#pragma unroll
        for (int s = 0; s < 4; ++s) f.v[s] *= a.scale;   // (what the stash zeroes it zeroes whatever the product is)
        return f;
      });
    }
    // ---- epilogue of the block, in the C/D layout of riab_mfma_slab.h: rows 8q + 4kh .. + 3 of tile mt are registers 4q .. 4q + 3
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int mb = mt * 32 + 8 * q + 4 * kh;
        // The groups of 4 bins are chained on the running sum, as gp_kernel chains them: left alone, the scheduler computes
        // every exponential of the block ahead of the serial state and keeps all of them live.
        float v[4] = {acc[mt][4 * q], acc[mt][4 * q + 1], acc[mt][4 * q + 2], acc[mt][4 * q + 3]};
        asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) : "v"(st.Z), "v"(st.m) : "memory");
        const v4f bias4 = *reinterpret_cast<const v4f*>(&s_bias[mb]);
        const v4f cx4 = *reinterpret_cast<const v4f*>(&s_cx[mb]);
        const v4f cy4 = *reinterpret_cast<const v4f*>(&s_cy[mb]);
        float mn = st.m;
        int an = st.arg;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[i] += bias4[i];
          if (v[i] > mn) {   // strictly greater, j ascending: the lowest index wins a tie; NaN never wins
            mn = v[i];
            an = m0 + mb + i;
          }
        }
        if (mn > st.m) {     // (st.m = -inf: exp2(-inf) = 0 times the zeros an empty state holds)
          const float sc = __builtin_amdgcn_exp2f((st.m - mn) * LOG2E);
          st.Z *= sc;
          st.sx *= sc;
          st.sy *= sc;
          st.m = mn;
          st.arg = an;
        }
        const float ms = st.m == neg_inf ? 0.0f : st.m;   // an empty state subtracts 0: -inf - -inf is never formed
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = __builtin_amdgcn_exp2f((v[i] - ms) * LOG2E);
          st.Z += p;
          st.sx = __builtin_fmaf(p, cx4[i], st.sx);
          st.sy = __builtin_fmaf(p, cy4[i], st.sy);
        }
      }
    }
  }
  // ---- the two half-waves of a column, low half first (the lanes kh = 0 hold it and write)
  const float m_o = __shfl_xor(st.m, 32), Z_o = __shfl_xor(st.Z, 32);
  const float sx_o = __shfl_xor(st.sx, 32), sy_o = __shfl_xor(st.sy, 32);
  const int arg_o = __shfl_xor(st.arg, 32);
  const bool take_o = m_o > st.m || (m_o == st.m && arg_o < st.arg);
  const float M = take_o ? m_o : st.m;
  int A = take_o ? arg_o : st.arg;
  A = A < a.J ? A : a.J - 1;
  const float Ms = M == neg_inf ? 0.0f : M;
  const float wa = __builtin_amdgcn_exp2f((st.m - Ms) * LOG2E), wb = __builtin_amdgcn_exp2f((m_o - Ms) * LOG2E);
  const float Z = __builtin_fmaf(Z_o, wb, st.Z * wa);
  const float sx = __builtin_fmaf(sx_o, wb, st.sx * wa);
  const float sy = __builtin_fmaf(sy_o, wb, st.sy * wa);
  const bool ok = Z > 0.0f && Z < INFINITY;   // (false for NaN)
  const float nan = __uint_as_float(0x7fc00000u);
  const int64_t b = b0 + wave * 32 + j;
  if (kh == 0 && b < a.B) {
    float* o = a.out + (int64_t)t * 6 * a.B + b;
    o[0] = ok ? sx / Z : nan;
    o[a.B] = ok ? sy / Z : nan;
    o[2 * a.B] = ok ? a.centres[A] : nan;
    o[3 * a.B] = ok ? a.centres[(int64_t)a.Jp + A] : nan;
    o[4 * a.B] = ok ? M + logf(Z) : nan;
    o[5 * a.B] = ok ? 1.0f / Z : nan;
  }
}

// counts[w][e] += rows[r][e] for the rows r of the piece that lie in window w; e indexes quads of (cell, lane) bytes.
__global__ __launch_bounds__(256) void window_counts_kernel(const uint32_t* rows, int64_t T, int64_t quads, int64_t row0,
                                                            int64_t window, int64_t w_first, int64_t n_w, uint32_t* counts) {
  const int64_t total = n_w * quads;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t w = w_first + i / quads, e = i % quads;
    int64_t r_lo = w * window - row0, r_hi = r_lo + window;
    r_lo = r_lo < 0 ? 0 : r_lo;
    r_hi = r_hi > T ? T : r_hi;
    uint32_t c = counts[w * quads + e];
    for (int64_t r = r_lo; r < r_hi; ++r) {
      const uint32_t s = rows[r * quads + e];
      const uint32_t even = ((c & 0x00ff00ffu) + (s & 0x00ff00ffu)) & 0x00ff00ffu;
      const uint32_t odd = (((c >> 8) & 0x00ff00ffu) + ((s >> 8) & 0x00ff00ffu)) & 0x00ff00ffu;
      c = even | (odd << 8);
    }
    counts[w * quads + e] = c;
  }
}

template <bool COUNTS>
void bayes_launch(int mt, dim3 grid, hipStream_t stream, const BayesArgs& a) {
  if (mt == 4) hipLaunchKernelGGL((bayes_kernel<4, COUNTS>), grid, dim3(256), 0, stream, a);
  else if (mt == 2) hipLaunchKernelGGL((bayes_kernel<2, COUNTS>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((bayes_kernel<1, COUNTS>), grid, dim3(256), 0, stream, a);
}

}  // namespace

extern "C" int riab_history_window_counts(const uint8_t* rows, int64_t T, int32_t n, int64_t B, int64_t row0, int32_t window,
                                          int64_t n_windows, uint8_t* counts, riab_stream_t stream) {
  if (!rows || !counts) return RIAB_EINVAL;
  if (window < 1 || window > RIAB_BAYES_MAX_WINDOW) return RIAB_EINVAL;
  if (T < 0 || n < 1 || B <= 0 || row0 < 0 || n_windows < 0) return RIAB_EINVAL;
  if (B & 3) return RIAB_EALIGN;
  if (((uintptr_t)rows | (uintptr_t)counts) & 3) return RIAB_EALIGN;
  const int64_t quads = (int64_t)n * (B / 4);   // (B < 2^63, n < 2^31: the product is checked against T below)
  if (quads >= 0x7fffffffLL || (T > 0 && quads > 0x7ffffffeLL / T)) return RIAB_ETOOBIG;
  if (row0 > 0x7fffffffffffLL - T) return RIAB_ETOOBIG;
  if (T == 0 || n_windows == 0) return RIAB_OK;
  const int64_t w_first = row0 / window;
  int64_t w_last = (row0 + T - 1) / window;
  if (w_last > n_windows - 1) w_last = n_windows - 1;
  if (w_first > w_last) return RIAB_OK;   // every row belongs to a window past the last one
  const int64_t n_w = w_last - w_first + 1;
  int64_t blocks = (n_w * quads + 255) / 256;   // (n_w <= T: below 2^31 - 1 by the check above)
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(window_counts_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint32_t*>(rows), T, quads, row0, (int64_t)window, w_first, n_w,
                     reinterpret_cast<uint32_t*>(counts));
  return (int)hipGetLastError();
}

extern "C" int riab_bayes_decode(const RiabFFInput* inputs, int32_t n_inputs, int32_t inputs_are_counts, float scale,
                                 const float* bias, const float* centres, int32_t J, int32_t Jp, int64_t T, int64_t B,
                                 float* out, int32_t block_tiles, riab_stream_t stream) {
  if (!inputs || !bias || !centres || !out) return RIAB_EINVAL;
  if (n_inputs < 1 || n_inputs > RIAB_FF_MAX_INPUTS || J < 1 || Jp < J || T < 0 || B <= 0) return RIAB_EINVAL;
  if (block_tiles != 0 && block_tiles != 1 && block_tiles != 2 && block_tiles != 4) return RIAB_EINVAL;
  if (!inputs_are_counts && !isfinite(scale)) return RIAB_EINVAL;
  BayesArgs a = {};
  for (int l = 0; l < n_inputs; ++l) {
    if (!inputs[l].rates || !inputs[l].wt || inputs[l].n_in < 1) return RIAB_EINVAL;
    a.rows[l] = inputs[l].rates;
    a.wt[l] = inputs[l].wt;
    a.n_in[l] = inputs[l].n_in;
  }
  if (J > RIAB_RATEMAP_MAX_BINS) return RIAB_EUNSUPPORTED;
  if ((B & 3) || (Jp & 31)) return RIAB_EALIGN;
  for (int l = 0; l < n_inputs; ++l)
    if (((uintptr_t)inputs[l].wt & 15) || ((uintptr_t)inputs[l].rates & (inputs_are_counts ? 3 : 15))) return RIAB_EALIGN;
  if (((uintptr_t)bias | (uintptr_t)centres | (uintptr_t)out) & 15) return RIAB_EALIGN;
  const int64_t tiles = (B + NB - 1) / NB;
  if (tiles > 0x7fffffffLL || T > 0x7fffffffLL / tiles) return RIAB_ETOOBIG;   // (a division: T * tiles could wrap)
  if (T == 0) return RIAB_OK;
  a.n_layers = n_inputs;
  a.bias = bias;
  a.centres = centres;
  a.J = J;
  a.Jp = Jp;
  a.B = B;
  a.tiles = (int)tiles;
  a.scale = scale;
  a.out = out;
  // bins per block: 128 (4 MFMA row tiles), 64 or 32 for small grids; block_tiles overrides (the bits do not depend on it)
  const int mt = block_tiles ? block_tiles : (Jp >= 128 ? 4 : Jp >= 64 ? 2 : 1);
  const dim3 grid((unsigned)(T * tiles));
  if (inputs_are_counts) bayes_launch<true>(mt, grid, (hipStream_t)stream, a);
  else bayes_launch<false>(mt, grid, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
