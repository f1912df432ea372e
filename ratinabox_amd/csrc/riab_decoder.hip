// riab_decoder.hip — the moment matrix a linear (ridge) decoder is fitted from, accumulated where the history lives.
//
// Replaces the host route of the reference's decoding workflow (tests/test_advanced.py::test_decoding_position, the
// decoding_position_example demo): history["firingrate"] and history["pos"] copied to the host and handed to
// sklearn.linear_model.Ridge.  Here every (step, agent) pair of the rows given is one sample of the AUGMENTED vector
//
//   z = [ rates of input 0 ; ... ; rates of input L-1 ; target rows of the trajectory record ; 1 ]      (m entries)
//
// and one call adds  sum_samples z z^T  to a float64 m x m matrix: X^T X, X^T y, the column sums and the sample count
// in one pass (what ratinabox_amd/_decoder.py solves the ridge system from).
//
//   moments_kernel   grid (pairs of 64-row blocks (I >= J) of z, splits of the samples).  A workgroup stages
//                    [64 rows][64 samples] fp32 slabs of its two row blocks in LDS (coalesced 16-byte loads, the next
//                    slab in flight while this one is multiplied), widens them to float64 once per operand and feeds
//                    v_mfma_f64_16x16x4_f64: the contraction index is the sample.  Each of the 4 waves owns 2 x 2 tiles
//                    of the 4 x 4 the block pair has; tiles above the diagonal are not computed.  The partial of a
//                    split goes to the workspace as float64.
//   finish_kernel    adds the splits' partials of an element in split order into moments[i][j] and its mirror.
//
// Why float64 on the matrix cores: ridge with an intercept centres the Gram matrix (G - N xbar xbar^T), which cancels
// about six digits at the conditioning of place-cell data; an fp32 accumulation moves the decoded position by a
// millimetre, float64 in any order by 1e-11 m.
//
// Masking: a padding lane (b >= n_real) or a sample with a non-finite target value is left out by SELECT while the slab
// is staged — every row of its column, the 1 included, is written as 0 — so whatever those lanes hold (NaN, 3e38)
// never reaches a product.  Determinism: the partition into splits depends on the shape alone, a wave adds its samples
// in slab order, the splits are added in split order; no floating-point atomic anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "riab_device.h"   // finite_bits

namespace {

using riab::finite_bits;

constexpr int kBlock = 256;
constexpr int kRows = 64;        // rows of z per block (4 tiles of 16)
constexpr int kSlab = 64;        // samples per slab
constexpr int kStride = 68;      // floats per LDS row: 16-byte aligned, and 68 = 4 mod 64 spreads 16 rows over all banks
constexpr int kRowsPerThread = kRows / (kBlock / 16);   // 4: a thread stages one 4-sample column group of these rows
constexpr int kMaxSplits = 16;

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct MomentArgs {
  const float* rows[RIAB_FF_MAX_INPUTS];
  int32_t n[RIAB_FF_MAX_INPUTS];
  int32_t first[RIAB_FF_MAX_INPUTS + 1];   // first row of z of each input; [n_inputs] = sum of n
  int32_t target_rows[RIAB_MOMENTS_MAX_TARGETS];
  int32_t n_inputs, n_targets, m;
};

// where row g of z comes from: a pointer to its value at step 0, lane 0 and its stride per step; or a constant
struct RowSource {
  const float* base;   // nullptr: the constant
  int64_t step;        // floats per history row
  float constant;      // 1 for the last row of z, 0 for the rows that pad m to the block
};

__device__ __forceinline__ RowSource row_source(const MomentArgs& a, const float* traj, int64_t B, int g) {
  RowSource s = {nullptr, 0, 0.0f};
  const int nx = a.first[a.n_inputs];
  if (g < nx) {
    int l = 0;
    while (g >= a.first[l + 1]) ++l;
    s.base = a.rows[l] + (int64_t)(g - a.first[l]) * B;
    s.step = (int64_t)a.n[l] * B;
  } else if (g < nx + a.n_targets) {
    s.base = traj + (int64_t)a.target_rows[g - nx] * B;
    s.step = (int64_t)RIAB_HIST_ROWS * B;
  } else if (g == a.m - 1) {
    s.constant = 1.0f;
  }
  return s;
}

__device__ __forceinline__ f32x4 select4(const bool* keep, f32x4 v) {
  f32x4 r;
  r.x = keep[0] ? v.x : 0.0f; r.y = keep[1] ? v.y : 0.0f; r.z = keep[2] ? v.z : 0.0f; r.w = keep[3] ? v.w : 0.0f;
  return r;
}

// One slab of one thread in registers: the values of its rows of both blocks for its 4 samples, already masked.
struct Staged {
  f32x4 a[kRowsPerThread], b[kRowsPerThread];
};

__global__ void __launch_bounds__(kBlock) moments_kernel(MomentArgs args, const float* __restrict__ traj, int64_t Tu,
                                                         int64_t t_step, int64_t B, int64_t n_real, int64_t slabs,
                                                         int32_t n_pairs, double* __restrict__ workspace,
                                                         unsigned long long* __restrict__ n_dropped) {
  __shared__ __attribute__((aligned(16))) float lds[2][kRows * kStride];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // block pair p -> (I, J), I >= J, p = I (I + 1) / 2 + J
  int I = 0;
  while ((I + 1) * (I + 2) / 2 <= (int)blockIdx.x) ++I;
  const int J = (int)blockIdx.x - I * (I + 1) / 2;
  const bool diagonal = I == J;
  float* slab_a = lds[0];
  float* slab_b = diagonal ? lds[0] : lds[1];

  const int quad = tid & 15, row0 = tid >> 4;   // this thread stages samples 4 quad .. 4 quad + 3 of rows row0 + 16 i
  RowSource src_a[kRowsPerThread], src_b[kRowsPerThread];
#pragma unroll
  for (int i = 0; i < kRowsPerThread; ++i) {
    src_a[i] = row_source(args, traj, B, I * kRows + row0 + 16 * i);
    src_b[i] = row_source(args, traj, B, J * kRows + row0 + 16 * i);
  }
  const int64_t slabs_per_row = (B + kSlab - 1) / kSlab;
  const int64_t s_begin = slabs * blockIdx.y / gridDim.y, s_end = slabs * (blockIdx.y + 1) / gridDim.y;
  const bool counts = blockIdx.x == 0 && row0 == 0;   // one thread per sample column of the whole launch counts the dropped

  auto fetch = [&](int64_t s, Staged& st) {
    const int64_t tu = s / slabs_per_row, bs = s - tu * slabs_per_row;
    const int64_t t = tu * t_step, b = bs * kSlab + 4 * quad;
    bool keep[4] = {false, false, false, false};
    if (b < B) {   // (B % 4 == 0: a column group is inside the row or outside it)
      int bad[4] = {0, 0, 0, 0};
#pragma unroll
      for (int d = 0; d < RIAB_MOMENTS_MAX_TARGETS; ++d) {
        if (d < args.n_targets) {
          const f32x4 y = *reinterpret_cast<const f32x4*>(traj + (t * RIAB_HIST_ROWS + args.target_rows[d]) * B + b);
          bad[0] |= !finite_bits(y.x); bad[1] |= !finite_bits(y.y); bad[2] |= !finite_bits(y.z); bad[3] |= !finite_bits(y.w);
        }
      }
      int dropped = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool real = b + j < n_real;
        keep[j] = real && !bad[j];
        dropped += real && bad[j];
      }
      if (counts && dropped) atomicAdd(n_dropped, (unsigned long long)dropped);   // (integer: exact in any order)
    }
    const bool any = keep[0] || keep[1] || keep[2] || keep[3];
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
      f32x4 va = {src_a[i].constant, src_a[i].constant, src_a[i].constant, src_a[i].constant};
      if (any && src_a[i].base) va = *reinterpret_cast<const f32x4*>(src_a[i].base + t * src_a[i].step + b);
      st.a[i] = select4(keep, va);
      if (!diagonal) {
        f32x4 vb = {src_b[i].constant, src_b[i].constant, src_b[i].constant, src_b[i].constant};
        if (any && src_b[i].base) vb = *reinterpret_cast<const f32x4*>(src_b[i].base + t * src_b[i].step + b);
        st.b[i] = select4(keep, vb);
      }
    }
  };
  auto stage = [&](const Staged& st) {
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
      *reinterpret_cast<f32x4*>(slab_a + (row0 + 16 * i) * kStride + 4 * quad) = st.a[i];
      if (!diagonal) *reinterpret_cast<f32x4*>(slab_b + (row0 + 16 * i) * kStride + 4 * quad) = st.b[i];
    }
  };

  // wave (wi, wj) owns tiles (2 wi + a, 2 wj + b), a, b in {0, 1}, of the 4 x 4 tiles of the block pair; on a diagonal
  // block the tiles above the diagonal are left out (wave-uniform)
  const int wi = wave >> 1, wj = wave & 1;
  bool live[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)   // (and so are the tiles that lie wholly in the rows that pad m to the block)
      live[a][b] = (!diagonal || 2 * wj + b <= 2 * wi + a) && I * kRows + (2 * wi + a) * 16 < args.m &&
                   J * kRows + (2 * wj + b) * 16 < args.m;
  const bool wave_live = live[0][0] || live[0][1] || live[1][0] || live[1][1];
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};

  // operand of lane l for tile row r0: row r0 + (l & 15), samples 16 (l >> 4) + j in "k step" j — both operands use the
  // same assignment of samples to k, which is all the contraction needs, and a lane reads 16 consecutive floats
  const int op_row = lane & 15, op_col = 16 * (lane >> 4);

  Staged st;
  if (s_begin < s_end) fetch(s_begin, st);
  for (int64_t s = s_begin; s < s_end; ++s) {
    __syncthreads();   // (the slab before this one has been read by every wave)
    stage(st);
    __syncthreads();
    if (s + 1 < s_end) fetch(s + 1, st);
    if (wave_live) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {   // 4 chunks of 4 k steps
        double wa[2][4], wb[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(slab_a + ((2 * wi + a) * 16 + op_row) * kStride + op_col + 4 * c);
          wa[a][0] = v.x; wa[a][1] = v.y; wa[a][2] = v.z; wa[a][3] = v.w;
          const f32x4 u = *reinterpret_cast<const f32x4*>(slab_b + ((2 * wj + a) * 16 + op_row) * kStride + op_col + 4 * c);
          wb[a][0] = u.x; wb[a][1] = u.y; wb[a][2] = u.z; wb[a][3] = u.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
              if (live[a][b]) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[a][k], wb[b][k], acc[a][b], 0, 0, 0);
      }
    }
  }

  // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg
  double* out = workspace + ((int64_t)blockIdx.y * n_pairs + blockIdx.x) * (kRows * kRows);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {   // (a tile left out stores its zeros: every double of the workspace is written)
      {
        const int r = (2 * wi + a) * 16 + (lane >> 4), cidx = (2 * wj + b) * 16 + (lane & 15);
        out[(r + 0) * kRows + cidx] = acc[a][b].x;
        out[(r + 4) * kRows + cidx] = acc[a][b].y;
        out[(r + 8) * kRows + cidx] = acc[a][b].z;
        out[(r + 12) * kRows + cidx] = acc[a][b].w;
      }
    }
}

// moments[i][j] (+ its mirror) += partial of split 0 + split 1 + ... in that order; one thread per element of a block pair
__global__ void __launch_bounds__(kBlock) moments_finish_kernel(const double* __restrict__ workspace, int32_t n_pairs,
                                                                int32_t splits, int32_t m, double* __restrict__ moments) {
  const int p = blockIdx.y;
  int I = 0;
  while ((I + 1) * (I + 2) / 2 <= p) ++I;
  const int J = p - I * (I + 1) / 2;
  const int e = blockIdx.x * kBlock + threadIdx.x;   // < 64 * 64
  const int i = I * kRows + e / kRows, j = J * kRows + e % kRows;
  if (i >= m || j > i) return;   // (j <= i < m; on a diagonal block only the computed tiles are read)
  const double* w = workspace + (int64_t)p * (kRows * kRows) + e;
  const int64_t stride = (int64_t)n_pairs * (kRows * kRows);
  double a = w[0];
  for (int s = 1; s < splits; ++s) a += w[s * stride];
  moments[(int64_t)i * m + j] += a;
  if (i != j) moments[(int64_t)j * m + i] += a;
}

int64_t used_rows(int64_t T, int64_t t_step) { return (T + t_step - 1) / t_step; }

int64_t slab_count(int64_t T, int64_t t_step, int64_t B) { return used_rows(T, t_step) * ((B + kSlab - 1) / kSlab); }

int64_t split_count(int64_t slabs) { return slabs < 1 ? 1 : (slabs < kMaxSplits ? slabs : kMaxSplits); }

int64_t pair_count(int32_t m) {
  const int64_t nb = (m + kRows - 1) / kRows;
  return nb * (nb + 1) / 2;
}

int check_shape(int64_t T, int64_t t_step, int32_t m, int64_t B) {
  if (T < 0 || t_step < 1 || m < 1 || B <= 0) return RIAB_EINVAL;
  if (B & 3) return RIAB_EALIGN;
  if (m > RIAB_MOMENTS_MAX_M || T * (B / 4) >= 0x7fffffffLL) return RIAB_ETOOBIG;
  return RIAB_OK;
}

}  // namespace

extern "C" int64_t riab_history_moments_workspace(int64_t T, int64_t t_step, int32_t m, int64_t B) {
  const int rc = check_shape(T, t_step, m, B);
  if (rc != RIAB_OK) return rc;
  return split_count(slab_count(T, t_step, B)) * pair_count(m) * (kRows * kRows);
}

extern "C" int riab_history_moments(const RiabMomentInput* inputs, int32_t n_inputs, const float* traj,
                                    const int32_t* target_rows, int32_t n_targets, int64_t T, int64_t t_step, int64_t B,
                                    int64_t n_real, double* moments, int64_t* n_dropped, double* workspace,
                                    riab_stream_t stream) {
  if (!inputs || !traj || !target_rows || !moments || !n_dropped || !workspace) return RIAB_EINVAL;
  if (n_inputs < 1 || n_inputs > RIAB_FF_MAX_INPUTS || n_targets < 1 || n_targets > RIAB_MOMENTS_MAX_TARGETS)
    return RIAB_EINVAL;
  if (T < 0 || t_step < 1 || B <= 0 || n_real < 0 || n_real > B) return RIAB_EINVAL;
  MomentArgs args = {};
  int64_t m = 0;
  for (int l = 0; l < n_inputs; ++l) {
    if (!inputs[l].rows || inputs[l].n < 1) return RIAB_EINVAL;
    args.rows[l] = inputs[l].rows;
    args.n[l] = inputs[l].n;
    args.first[l] = (int32_t)m;
    m += inputs[l].n;
    if (m > RIAB_MOMENTS_MAX_M) return RIAB_ETOOBIG;
  }
  args.first[n_inputs] = (int32_t)m;
  for (int d = 0; d < n_targets; ++d) {
    if (target_rows[d] < 0 || target_rows[d] >= RIAB_HIST_ROWS) return RIAB_EINVAL;
    args.target_rows[d] = target_rows[d];
  }
  m += n_targets + 1;
  args.n_inputs = n_inputs;
  args.n_targets = n_targets;
  args.m = (int32_t)m;
  if (B & 3) return RIAB_EALIGN;
  for (int l = 0; l < n_inputs; ++l)
    if ((uintptr_t)inputs[l].rows & 15) return RIAB_EALIGN;
  if (((uintptr_t)traj & 15) || ((uintptr_t)moments & 7) || ((uintptr_t)n_dropped & 7) || ((uintptr_t)workspace & 7))
    return RIAB_EALIGN;
  const int rc = check_shape(T, t_step, (int32_t)m, B);
  if (rc != RIAB_OK) return rc;
  if (T == 0) return RIAB_OK;
  const int64_t slabs = slab_count(T, t_step, B), splits = split_count(slabs), pairs = pair_count((int32_t)m);
  hipLaunchKernelGGL(moments_kernel, dim3((unsigned)pairs, (unsigned)splits), dim3(kBlock), 0, (hipStream_t)stream, args, traj,
                     used_rows(T, t_step), t_step, B, n_real, slabs, (int32_t)pairs, workspace,
                     reinterpret_cast<unsigned long long*>(n_dropped));
  int err = (int)hipGetLastError();
  if (err) return err;
  hipLaunchKernelGGL(moments_finish_kernel, dim3(kRows * kRows / kBlock, (unsigned)pairs), dim3(kBlock), 0,
                     (hipStream_t)stream, workspace, (int32_t)pairs, (int32_t)splits, (int32_t)m, moments);
  return (int)hipGetLastError();
}
