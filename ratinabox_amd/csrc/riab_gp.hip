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
  float* out;             // [T][D][B]
};

// 3 waves per SIMD (<= 168 registers; 35 KB of LDS) keep 3 workgroups on a CU, as ff_kernel has them: the stash and
// barrier of one and the epilogue of another hide behind the MFMAs of the third.
template <int MT>
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
    if (kh == 0 && b < a.B && d < a.D) a.out[((int64_t)t * a.D + d) * a.B + b] = v;
  }
}

}  // namespace

extern "C" int riab_gp_predict(const RiabFFInput* inputs, int32_t n_inputs, const float* sq_train, const float* alpha,
                               int32_t n_out, int32_t n_train, float inv_two_ell2, int64_t T, int64_t B, float* out,
                               riab_stream_t stream) {
  if (!inputs || !sq_train || !alpha || !out) return RIAB_EINVAL;
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
  // training samples per block: 128 (4 MFMA row tiles), 64 or 32 for small training sets
  const dim3 grid((unsigned)(T * tiles));
  if (a.Np >= 128) hipLaunchKernelGGL(gp_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else if (a.Np >= 64) hipLaunchKernelGGL(gp_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(gp_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
