// riab_gp.hip — the predictive mean of a Gaussian-process decoder (RBF kernel) over history rows, in one fused kernel.
//
// The reference decodes position with sklearn.gaussian_process.GaussianProcessRegressor(alpha, RBF(l)) beside its Ridge
// (tests/test_advanced.py::test_decoding_position, the decoding demo).  Once fitted, the decoder is N training vectors
// x_j and D dual coefficient rows alpha_d (ratinabox_amd/_gp_decoder.py solves them), and decoding a sample x* is
//
//     mean_d(x*) = sum_{j < N} exp(-|x* - x_j|^2 / (2 l^2)) * alpha_d[j]
//
// for every (row, agent) sample of a history: M = T * B queries against N training samples of n cells.  With
// |x* - x_j|^2 = |x*|^2 + |x_j|^2 - 2 x*.x_j the cross term is a GEMM, which runs on the streamed core of
// csrc/riab_mfma_slab.h (layouts, bounds and barriers are stated there): the training matrix is operand A, the positions
// are the columns.
//
//   gp_kernel<MT>   grid (position tiles of 128 x T).  A workgroup of 4 waves owns 128 positions of one row.  The training
//                   samples are walked in blocks of 32 MT; for each block the whole K (every input population) is
//                   contracted into MT accumulator tiles, |x*|^2 is summed from the rate fragments the MFMAs are fed with
//                   anyway (the core's per-fragment hook), and the epilogue turns each accumulator into
//                   exp(-max(0, d2) / (2 l^2)) and multiplies it into D running sums.  The M x N matrix lives in
//                   accumulator registers only.
//   gp_kernel<MT, true> + gp_var_kernel<MT>   the predictive variance 1 - |L^-1 k*|^2 (riab_gp_predict_var): the same
//                   kernel also stores its k to a workspace [T][Np][B], and a second kernel on the same grid contracts
//                   the transposed L^-1 with it over the triangular half and sums the squares.  Stated at the kernels.
//
// Arithmetic of one position, in order: for each training block, dot_j = the k-ordered fmaf chain of the MFMA; sq* = the
// k-ordered fmaf chains of the two half-waves, added; d2 = fma(-2, dot_j, sq* + sq_j), clamped at 0 by a select that
// keeps NaN; k = exp2(-(d2 * inv_two_ell2) * log2 e) (v_exp_f32); sum_d = fma(k, alpha_d[j], sum_d) with j ascending
// within each half-wave (rows 4h..4h+3 of every group of 8), and the two halves added at the end, low half first.
// Nothing of this depends on T, B, the tile or the lane, nor on MT (a block of 32 MT samples is walked in the order of
// j), so a row decoded alone has the bits it has inside a many-row call.  No atomics, no workspace: N is not split.
//
// Columns are independent: whatever a padding lane holds stays in its own column of the MFMA and of the epilogue.  A
// column whose |x*|^2 is not finite (a NaN, an infinity or an overflowing rate) is written as NaN.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "riab_device.h"   // finite_bits, LOG2E
#include "riab_mfma_slab.h"

namespace {

using namespace riab;

constexpr int GP_MAX_D = 4;

struct GPArgs {
  const float* rates[RIAB_FF_MAX_INPUTS];  // [T][n_in][B]
  const float* wt[RIAB_FF_MAX_INPUTS];     // [n_in][Np]: the training matrix of the population, transposed
  int n_in[RIAB_FF_MAX_INPUTS];
  int n_layers;
  const float* sq_train;  // [Np]
  const float* alpha;     // [D][Np]
  int D, Np;
  int64_t B;
  int tiles;              // position tiles per row
  float inv_two_ell2;
  float* out;             // [T][D][B] (gp_kernel<MT, true>: may be null)
  float* kstar;           // gp_kernel<MT, true>: [T][Np][B], the kernel values k*_j of every position
};

// 3 waves per SIMD (<= 168 registers; 35 KB of LDS) keep 3 workgroups on a CU, as ff_kernel has them: the stash and
// barrier of one and the epilogue of another hide behind the MFMAs of the third.
//
// STORE_K (stage 1 of riab_gp_predict_var): the block epilogue also stores every k it computes to kstar[t][j][b], rows
// j < Np only (a block of 32 MT samples may reach past Np), NaN in every row of a column whose |x*|^2 is not finite
// (left alone, an infinite |x*|^2 gives k = 0).  The sums are the same instructions in the same order.
template <int MT, bool STORE_K = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void gp_kernel(const GPArgs a) {
  __shared__ __align__(16) SlabTiles<MT> lds;                     // training slab (A) and rates slab
  __shared__ __align__(16) float s_sq[MT * 32];                   // |x_j|^2 of the training block
  __shared__ __align__(16) float s_al[GP_MAX_D][MT * 32];         // alpha rows of the training block (rows >= D: 0)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = blockIdx.x / a.tiles;
  const int64_t b0 = (int64_t)(blockIdx.x - t * a.tiles) * NB;

  const SlabRole<MT> role(lds, tid, wave);
  const Frag<MT> fr(lane, wave);
  const bool is_b = role.is_b;
  const bool b_ok = b0 + role.c4 < a.B;
  const int64_t ld = is_b ? a.B : (int64_t)a.Np;
  const int kh = fr.kh, j = fr.j;

  float sum[GP_MAX_D] = {0.0f, 0.0f, 0.0f, 0.0f};
  float sq_q = 0.0f;
  int buf = 0;
  for (int m0 = 0; m0 < a.Np; m0 += MT * 32) {   // training blocks
    const SlabMask mask = {is_b ? b_ok : role.a_quad_ok(m0, a.Np), 4};
    const int64_t col = mask.col_ok ? (is_b ? b0 + role.c4 : (int64_t)m0 + role.c4) : 0;
    v16f acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) zero_acc(acc[i]);
    float sq_half = 0.0f;   // this half-wave's share of |x*|^2: k = 8g + 2s + kh, ascending
    for (int l = 0; l < a.n_layers; ++l) {
      const int K = a.n_in[l];
      const float* src = is_b ? a.rates[l] + (int64_t)t * K * a.B : a.wt[l];
      __syncthreads();  // the slab and the epilogue tables before this have been consumed
      if (l == 0 && tid < MT * 32) {
        const bool in = m0 + tid < a.Np;
        s_sq[tid] = in ? a.sq_train[m0 + tid] : 0.0f;
#pragma unroll
        for (int d = 0; d < GP_MAX_D; ++d) s_al[d][tid] = (in && d < a.D) ? a.alpha[(int64_t)d * a.Np + m0 + tid] : 0.0f;
      }
      contract_population(
          lds, role, fr, buf, K, mask, acc, [&](int kbase) { return fetch_f32(src, ld, col, K, kbase); },
          [&](float x) { sq_half = __builtin_fmaf(x, x, sq_half); });
    }
    // |x*|^2 of the lane's position: the two half-waves hold the even and the odd k (the sum commutes: both halves get
    // the same bits).  Every training block computes the same value again.
    sq_q = sq_half + __shfl_xor(sq_half, 32);
    const bool k_nan = STORE_K && !finite_bits(sq_q);
    const int64_t kb = b0 + wave * 32 + j;   // the lane's position
    // ---- epilogue of the block, in the C/D layout of riab_mfma_slab.h: rows 8q + 4kh .. + 3 of tile mt are registers 4q .. 4q + 3
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int mb = mt * 32 + 8 * q + 4 * kh;
        // The groups of 4 samples are chained: a group's dot products become available only once the sums of the group
        // before it are, and its table reads stay behind that point.  Left alone, the scheduler computes all 16 MT
        // exponentials ahead of the serial sums and keeps every one of them (and the 20 table registers of every
        // group) live, which costs the occupancy the main loop needs.
        float dot[4] = {acc[mt][4 * q], acc[mt][4 * q + 1], acc[mt][4 * q + 2], acc[mt][4 * q + 3]};
        asm volatile("" : "+v"(dot[0]), "+v"(dot[1]), "+v"(dot[2]), "+v"(dot[3])
                     : "v"(sum[0]), "v"(sum[1]), "v"(sum[2]), "v"(sum[3]) : "memory");
        const v4f sq4 = *reinterpret_cast<const v4f*>(&s_sq[mb]);
        v4f al[GP_MAX_D];
#pragma unroll
        for (int d = 0; d < GP_MAX_D; ++d) al[d] = *reinterpret_cast<const v4f*>(&s_al[d][mb]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float d2 = __builtin_fmaf(-2.0f, dot[i], sq_q + sq4[i]);
          d2 = d2 < 0.0f ? 0.0f : d2;   // (a select, not fmaxf: NaN stays NaN)
          const float k = __builtin_amdgcn_exp2f(-(d2 * a.inv_two_ell2) * LOG2E);
          if constexpr (STORE_K) {
            const int jr = m0 + mb + i;
            if (jr < a.Np && kb < a.B) a.kstar[((int64_t)t * a.Np + jr) * a.B + kb] = k_nan ? __uint_as_float(0x7fc00000u) : k;
          }
#pragma unroll
          for (int d = 0; d < GP_MAX_D; ++d) sum[d] = __builtin_fmaf(k, al[d][i], sum[d]);
        }
      }
    }
  }
  const bool poisoned = !finite_bits(sq_q);
  const int64_t b = b0 + wave * 32 + j;
#pragma unroll
  for (int d = 0; d < GP_MAX_D; ++d) {
    const float hi = __shfl_xor(sum[d], 32);
    const float v = poisoned ? __uint_as_float(0x7fc00000u) : sum[d] + hi;
    if (kh == 0 && b < a.B && d < a.D && (!STORE_K || a.out)) a.out[((int64_t)t * a.D + d) * a.B + b] = v;
  }
}

// Stage 2 of riab_gp_predict_var: var[t][b] = 1 - sum_i (sum_j linv_t[j][i] kstar[t][j][b])^2.  gp_kernel's loop with
// other operands: operand A is linv_t ([k = j][m = i], (L^-1)[i][j], zero for j > i), the "population" is the workspace
// (K rows of positions).  The rows i are walked in blocks of 32 MT; for the block starting at m0 every linv_t[j][i] with
// j >= m0 + 32 MT is zero, so the contraction stops there: K = min(m0 + 32 MT, Np), and the rows of linv_t at or past K
// are never read for this block's columns (the core's clamped fetch reads row K - 1 in their place and masks it).
//
// Arithmetic of one position, in order: acc_i = the j-ordered fmaf chain of the MFMA over j < K.  Its terms with j > i
// are 0 * k*_j with k*_j finite or NaN in a whole column, so they change nothing and acc_i does not depend on where the
// block (hence MT) ends the chain.  sumsq = fma(acc_i, acc_i, sumsq) with i ascending within each half-wave (rows
// 4h..4h+3 of every group of 8), the halves added at the end, low half first: the order of gp_kernel's sums.  Rows i >=
// Np of a block that reaches past Np are masked columns of A: acc_i = 0.  var = 1 - sumsq, 0 where negative by a select
// that keeps NaN; a poisoned column is NaN in every row of the workspace, so every acc_i (linv_t[0][0] > 0) and var are.
template <int MT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void gp_var_kernel(
    const float* __restrict__ linv_t, const float* __restrict__ kstar, int Np, int64_t B, int tiles,
    float* __restrict__ out_var) {
  __shared__ __align__(16) SlabTiles<MT> lds;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = blockIdx.x / tiles;
  const int64_t b0 = (int64_t)(blockIdx.x - t * tiles) * NB;

  const SlabRole<MT> role(lds, tid, wave);
  const Frag<MT> fr(lane, wave);
  const bool is_b = role.is_b;
  const bool b_ok = b0 + role.c4 < B;
  const int64_t ld = is_b ? B : (int64_t)Np;
  const float* src = is_b ? kstar + (int64_t)t * Np * B : linv_t;

  float sumsq = 0.0f;
  int buf = 0;
  for (int m0 = 0; m0 < Np; m0 += MT * 32) {   // blocks of rows of L^-1
    const int K = m0 + MT * 32 < Np ? m0 + MT * 32 : Np;
    const SlabMask mask = {is_b ? b_ok : role.a_quad_ok(m0, Np), 4};
    const int64_t col = mask.col_ok ? (is_b ? b0 + role.c4 : (int64_t)m0 + role.c4) : 0;
    v16f acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) zero_acc(acc[i]);
    __syncthreads();  // the slab before this has been consumed
    contract_population(lds, role, fr, buf, K, mask, acc, [&](int kbase) { return fetch_f32(src, ld, col, K, kbase); });
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) sumsq = __builtin_fmaf(acc[mt][r], acc[mt][r], sumsq);
  }
  const float total = sumsq + __shfl_xor(sumsq, 32);
  float v = 1.0f - total;
  v = v < 0.0f ? 0.0f : v;   // (a select, not fmaxf: NaN stays NaN)
  const int64_t b = b0 + wave * 32 + fr.j;
  if (fr.kh == 0 && b < B) out_var[(int64_t)t * B + b] = v;
}

}  // namespace

// The checks and the launch of gp_kernel that riab_gp_predict and riab_gp_predict_var share.  linv_t null: the mean alone
// (gp_kernel<MT>, `out` required); otherwise stage 1 (gp_kernel<MT, true>, `out` may be null) and stage 2.
static int gp_launch(const RiabFFInput* inputs, int32_t n_inputs, const float* sq_train, const float* alpha, int32_t n_out,
                     int32_t n_train, float inv_two_ell2, const float* linv_t, int64_t T, int64_t B, float* workspace,
                     float* out_var, float* out, riab_stream_t stream) {
  const bool var = linv_t != nullptr;   // (riab_gp_predict_var has refused a null linv_t, workspace or out_var)
  if (!inputs || !sq_train || !alpha || (!var && !out)) return RIAB_EINVAL;
  if (n_inputs < 1 || n_inputs > RIAB_FF_MAX_INPUTS || n_out < 1 || n_out > RIAB_GP_MAX_OUT) return RIAB_EINVAL;
  if (n_train < 1 || T < 0 || B <= 0) return RIAB_EINVAL;
  if (!(inv_two_ell2 > 0.0f) || !isfinite(inv_two_ell2)) return RIAB_EINVAL;
  if (n_train > RIAB_GP_MAX_TRAIN) return RIAB_ETOOBIG;
  GPArgs a = {};
  for (int l = 0; l < n_inputs; ++l) {
    if (!inputs[l].rates || !inputs[l].wt || inputs[l].n_in < 1) return RIAB_EINVAL;
    a.rates[l] = inputs[l].rates;
    a.wt[l] = inputs[l].wt;
    a.n_in[l] = inputs[l].n_in;
  }
  if (B & 3) return RIAB_EALIGN;
  for (int l = 0; l < n_inputs; ++l)
    if (((uintptr_t)inputs[l].rates | (uintptr_t)inputs[l].wt) & 15) return RIAB_EALIGN;
  if (((uintptr_t)sq_train | (uintptr_t)alpha | (uintptr_t)out) & 15) return RIAB_EALIGN;
  if (((uintptr_t)linv_t | (uintptr_t)workspace | (uintptr_t)out_var) & 15) return RIAB_EALIGN;
  const int64_t tiles = (B + NB - 1) / NB;
  if (tiles > 0x7fffffffLL || T > 0x7fffffffLL / tiles) return RIAB_ETOOBIG;   // (a division: T * tiles could wrap)
  if (T == 0) return RIAB_OK;
  a.n_layers = n_inputs;
  a.sq_train = sq_train;
  a.alpha = alpha;
  a.D = n_out;
  a.Np = (n_train + 31) / 32 * 32;
  a.B = B;
  a.tiles = (int)tiles;
  a.inv_two_ell2 = inv_two_ell2;
  a.out = out;
  a.kstar = workspace;
  // training samples per block: 128 (4 MFMA row tiles), 64 or 32 for small training sets
  const dim3 grid((unsigned)(T * tiles));
  const hipStream_t s = (hipStream_t)stream;
  if (!var) {
    if (a.Np >= 128) hipLaunchKernelGGL(gp_kernel<4>, grid, dim3(256), 0, s, a);
    else if (a.Np >= 64) hipLaunchKernelGGL(gp_kernel<2>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(gp_kernel<1>, grid, dim3(256), 0, s, a);
    return (int)hipGetLastError();
  }
  if (a.Np >= 128) {
    hipLaunchKernelGGL((gp_kernel<4, true>), grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(gp_var_kernel<4>, grid, dim3(256), 0, s, linv_t, workspace, a.Np, B, a.tiles, out_var);
  } else if (a.Np >= 64) {
    hipLaunchKernelGGL((gp_kernel<2, true>), grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(gp_var_kernel<2>, grid, dim3(256), 0, s, linv_t, workspace, a.Np, B, a.tiles, out_var);
  } else {
    hipLaunchKernelGGL((gp_kernel<1, true>), grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(gp_var_kernel<1>, grid, dim3(256), 0, s, linv_t, workspace, a.Np, B, a.tiles, out_var);
  }
  return (int)hipGetLastError();
}

extern "C" int riab_gp_predict(const RiabFFInput* inputs, int32_t n_inputs, const float* sq_train, const float* alpha,
                               int32_t n_out, int32_t n_train, float inv_two_ell2, int64_t T, int64_t B, float* out,
                               riab_stream_t stream) {
  return gp_launch(inputs, n_inputs, sq_train, alpha, n_out, n_train, inv_two_ell2, nullptr, T, B, nullptr, nullptr, out,
                   stream);
}

extern "C" int riab_gp_predict_var(const RiabFFInput* inputs, int32_t n_inputs, const float* sq_train, const float* alpha,
                                   int32_t n_out, int32_t n_train, float inv_two_ell2, const float* linv_t, int64_t T,
                                   int64_t B, float* workspace, float* out_var, float* out_mean, riab_stream_t stream) {
  if (!linv_t || !workspace || !out_var) return RIAB_EINVAL;
  return gp_launch(inputs, n_inputs, sq_train, alpha, n_out, n_train, inv_two_ell2, linv_t, T, B, workspace, out_var,
                   out_mean, stream);
}
