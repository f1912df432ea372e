// riab_gp.hip — the predictive mean of a Gaussian-process decoder (RBF kernel) over history rows, in one fused kernel.
//
// The reference decodes position with sklearn.gaussian_process.GaussianProcessRegressor(alpha, RBF(l)) beside its Ridge
// (tests/test_advanced.py::test_decoding_position, the decoding demo).  Once fitted, the decoder is N training vectors
// x_j and D dual coefficient rows alpha_d (ratinabox_amd/_gp_decoder.py solves them), and decoding a sample x* is
//
//     mean_d(x*) = sum_{j < N} exp(-|x* - x_j|^2 / (2 l^2)) * alpha_d[j]
//
// for every (row, agent) sample of a history: M = T * B queries against N training samples of n cells.  With
// |x* - x_j|^2 = |x*|^2 + |x_j|^2 - 2 x*.x_j the cross term is a GEMM, which is riab_feedforward's main loop
// (csrc/riab_ff.hip): the training matrix takes the place of W^T, the positions are the columns.
//
//   gp_kernel<MT>   grid (position tiles of 128 x T).  A workgroup of 4 waves owns 128 positions of one row; wave w owns
//                   positions [32w, 32w + 32).  The training samples are walked in blocks of 32 MT; for each block the
//                   whole K (every input population, slabs of 16 through double-buffered LDS) is contracted on
//                   v_mfma_f32_32x32x2_f32 into MT accumulator tiles, |x*|^2 is summed from the rate fragments the MFMAs
//                   are fed with anyway, and the epilogue turns each accumulator into exp(-max(0, d2) / (2 l^2)) and
//                   multiplies it into D running sums.  The M x N matrix lives in accumulator registers only.
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

#include "riab_hip.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int GP_KT = 16;    // K slab
constexpr int GP_NB = 128;   // positions per block
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

// One thread's share of a K slab, as in ff_kernel: waves 0-1 fetch the training matrix, waves 2-3 the rates; a thread
// takes rows kbase + 2s (s = 0..3) x 4 consecutive columns.  Rows past K read row K - 1 and columns outside the problem
// column 0 (both zeroed by the stash), so the fetch is branch-free and in bounds.
struct GPSlab {
  v4f v[4];
};

__device__ __forceinline__ GPSlab gp_fetch(const float* src, int64_t ld, int64_t col, int K, int kbase) {
  GPSlab f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int k = kbase + 2 * s;
    const int kc = k < K ? k : K - 1;
    f.v[s] = *reinterpret_cast<const v4f*>(src + (int64_t)kc * ld + col);
  }
  return f;
}

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// 3 waves per SIMD (<= 168 registers; 35 KB of LDS) keep 3 workgroups on a CU, as ff_kernel has them: the stash and
// barrier of one and the epilogue of another hide behind the MFMAs of the third.
template <int MT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void gp_kernel(const GPArgs a) {
  // LDS slab layout [g][kh][column][s] (k = 8g + 2s + kh), columns XOR-swizzled, double-buffered: ff_kernel's
  __shared__ __align__(16) float s_a[2][GP_KT / 4][MT * 32][4];   // training slab
  __shared__ __align__(16) float s_b[2][GP_KT / 4][GP_NB][4];     // rates slab
  __shared__ __align__(16) float s_sq[MT * 32];                   // |x_j|^2 of the training block
  __shared__ __align__(16) float s_al[GP_MAX_D][MT * 32];         // alpha rows of the training block (rows >= D: 0)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = blockIdx.x / a.tiles;
  const int64_t b0 = (int64_t)(blockIdx.x - t * a.tiles) * GP_NB;

  const bool is_b = wave >= 2;                           // wave-uniform
  const int c4 = (tid & 31) * 4, rg = (tid >> 5) & 3;    // rg = 2g + kh
  const int krow = (rg >> 1) * 8 + (rg & 1);
  const bool b_ok = b0 + c4 < a.B;                       // (B % 4 == 0: a float4 is wholly inside or outside)
  const int64_t ld = is_b ? a.B : (int64_t)a.Np;
  const int sw = (c4 >> 3) & 7;
  float* const s_dst = is_b ? &s_b[0][rg][0][0] : &s_a[0][rg][0][0];
  const int buf_stride = is_b ? (GP_KT / 4) * GP_NB * 4 : (GP_KT / 4) * MT * 32 * 4;
  const int kh = lane >> 5, j = lane & 31;
  const int jb = (wave * 32 + j) ^ (((wave * 32 + j) >> 3) & 7);
  int ja[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) ja[mt] = (mt * 32 + j) ^ (((mt * 32 + j) >> 3) & 7);

  float sum[GP_MAX_D] = {0.0f, 0.0f, 0.0f, 0.0f};
  float sq_q = 0.0f;
  int buf = 0;
  for (int m0 = 0; m0 < a.Np; m0 += MT * 32) {   // training blocks
    const bool col_ok = is_b ? b_ok : (c4 < MT * 32 && m0 + c4 < a.Np);
    const int64_t col = col_ok ? (is_b ? b0 + c4 : (int64_t)m0 + c4) : 0;
    // 4x4 register transpose [s][column] -> [column][s]; rows >= K and columns outside the problem become 0
    auto stash = [&](const GPSlab& f, int to, int K, int k0) {
      if (!is_b && c4 >= MT * 32) return;
      v4f v[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) v[s] = (col_ok && k0 + krow + 2 * s < K) ? f.v[s] : v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<v4f*>(s_dst + to * buf_stride + ((c4 + i) ^ sw) * 4) = v4f{v[0][i], v[1][i], v[2][i], v[3][i]};
    };
    v16f acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
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
      stash(gp_fetch(src, ld, col, K, krow), buf, K, 0);
      __syncthreads();
      for (int k0 = 0; k0 < K; k0 += GP_KT) {
        const bool more = k0 + GP_KT < K;  // block-uniform
        GPSlab nxt;
        if (more) nxt = gp_fetch(src, ld, col, K, k0 + GP_KT + krow);
#pragma unroll
        for (int g = 0; g < GP_KT / 8; ++g) {
          const v4f bq = *reinterpret_cast<const v4f*>(&s_b[buf][2 * g + kh][jb][0]);
          v4f aq[MT];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) aq[mt] = *reinterpret_cast<const v4f*>(&s_a[buf][2 * g + kh][ja[mt]][0]);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            sq_half = __builtin_fmaf(bq[s], bq[s], sq_half);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[mt][s], bq[s], acc[mt], 0, 0, 0);
          }
        }
        if (more) {
          stash(nxt, buf ^ 1, K, k0 + GP_KT);  // the other buffer was last read one iteration ago (barrier below)
          __syncthreads();
          buf ^= 1;
        }
      }
    }
    // |x*|^2 of the lane's position: the two half-waves hold the even and the odd k (the sum commutes: both halves get
    // the same bits).  Every training block computes the same value again.
    sq_q = sq_half + __shfl_xor(sq_half, 32);
    // ---- epilogue of the block: C/D layout col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
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
          const float k = __builtin_amdgcn_exp2f(-(d2 * a.inv_two_ell2) * 1.44269504088896341f);
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
  const int64_t tiles = (B + GP_NB - 1) / GP_NB;
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
