// contribs.NeuralNetworkNeurons for gfx950: a whole multi-layer perceptron in one launch.
//
//     h_0 = concat_l I_l          h_i = act_i(W_i h_{i-1} + bias_i)          out = h_L
//
// N = positions (agents x time rows), as in riab_ff.hip; a wave owns 32 positions and ALL rows of every layer.  On the fp32
// matrix cores (v_mfma_f32_32x32x2_f32: exact fp32), lane l = 32 kh + j, in the fragment layout of riab_mfma_slab.h.
//
// Layer 0 streams from memory as that header describes (K slabs of 16, double-buffered in LDS, swizzled columns, clamped
// fetches zeroed in the stash, two barriers per slab pair), with its types and swizzle() but a loop of its own: the A tile
// is a fixed 128 rows, the rates tile 32 nw positions, and the weights are torch.nn.Linear.weight read in place ([n_out][n_in], k contiguous), so a thread's 16-byte
// fetch of W is four consecutive k of one row; a slab maps k = 4 rg + s to (LDS row group rg, element s) for both operands
// and the W stash needs no transpose (the rates stash keeps ff_kernel's 4x4 register transpose).
//
// Layers >= 1 never touch LDS: the C/D fragment of a layer holds, per lane, rows of the lane's own column, and the
// contraction over k is order-free.  MFMA step (tile mi, reg r) takes as B the accumulator register r of tile mi as it
// stands: the low half-wave supplies row k = 32 mi + (r&3) + 8 (r>>2), the high half-wave row k + 4, and A is loaded with
// the matching k (lane (i, kh) reads W[m0 + i][k + 4 kh]: registers r = 4q..4q+3 are one 16-byte read).  No barrier, no
// LDS, no global memory between layers.  A wave's A reads are the layer's whole weight matrix (<= 64 KB, L2 resident).
//
// Block = nw waves (nw = 4 or 1, chosen by the host per launch: blockDim.x), position tile 32 nw.  The per-position
// arithmetic does not depend on nw, T, B or the tile's place: for a given network one kernel (one set of instructions;
// the instantiation follows from the layer widths alone) serves every launch, whatever its grid.
#include <type_traits>

#include "riab_act.h"
#include "riab_device.h"
#include "riab_mfma_slab.h"   // v4f, v16f, KT, swizzle()
#include "riab_mlp_logic.h"   // MLP_MAX_INPUTS, MLP_A_FLOATS; what the host decides per call (mlp_decide)

namespace riab {

static_assert(MLP_KT == KT, "riab_mlp_logic.h sizes the LDS slabs for riab_mfma_slab.h's KT");

struct MLPLayerArgs {
  const float* w;     // [n_out][n_in]
  const float* bias;  // [n_out] or null
  int n_in, n_out;
  int act;
  int vec;            // rows of w can be read 16 bytes at a time (base 16-byte aligned, n_in % 4 == 0)
  float p0, p1, p2, p3;
};

struct MLPArgs {
  const float* rates[MLP_MAX_INPUTS];  // [T][n][B]
  int n[MLP_MAX_INPUTS];               // cells of input l ...
  int koff[MLP_MAX_INPUTS];            // ... which are columns [koff, koff + n) of layer 0's w
  int vec0[MLP_MAX_INPUTS];            // layer 0's w can be read 16 bytes at a time at this input's columns
  int n_inputs, n_layers;
  MLPLayerArgs layer[RIAB_MLP_MAX_LAYERS];
  int64_t B;
  float* out;  // [T][n_out of the last layer][B]
};

// Four consecutive k of one row of W: W[m][c .. c+3], elements outside the matrix are 0.
// BOUNDS (w carries no padding: every address must lie in [w, w + n_out*n_in)).  The row is clamped to mc <= n_out - 1.
//  VEC: the caller guarantees w % 16 == 0, n_in % 4 == 0 and c % 4 == 0, so c < n_in implies c + 3 < n_in; a column group
//       with c >= n_in is redirected to c = 0 (n_in >= 4 here).  The read covers [mc*n_in + cc, mc*n_in + cc + 4) with
//       cc + 4 <= n_in: inside row mc, and 16-byte aligned.
//  else: element e reads column min(c + e, n_in - 1) of row mc, 4 bytes: inside row mc.
// What was redirected is zeroed afterwards ("the stash"), so the MFMA sees 0 for every k >= n_in and every row >= n_out.
template <bool VEC>
__device__ __forceinline__ v4f mlp_w4(const float* w, int n_in, int n_out, int m, int c, int c_end) {
  const bool m_ok = m < n_out;
  const float* row = w + (int64_t)(m_ok ? m : n_out - 1) * n_in;
  v4f v;
  if constexpr (VEC) {
    const bool ok = c < c_end;
    v = *reinterpret_cast<const v4f*>(row + (ok ? c : 0));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (m_ok && c + e < c_end) ? v[e] : 0.0f;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ok = c + e < c_end;
      const float x = row[ok ? c + e : n_in - 1];
      v[e] = (m_ok && ok) ? x : 0.0f;
    }
  }
  return v;
}

// Layer 0, rows [m0, m0 + 32 MT) x the block's positions, accumulated over every input population.
template <int MT, int MAXT>
__device__ __forceinline__ void mlp_first_layer(const MLPArgs& a, float* smem, int m0, int t, int64_t b0, int nw,
                                                v16f (&acc)[MAXT]) {
  static_assert(MT <= MAXT, "tile count");
  const int tid = threadIdx.x, lane = tid & 63, nt = nw * 64, nb = nw * 32;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* const s_a = smem;                 // [2][4][128][4]
  float* const s_b = smem + MLP_A_FLOATS;  // [2][4][nb][4]
  const MLPLayerArgs& L = a.layer[0];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

  // rates role (threads < nb): row group rg_b, 4 consecutive positions; rows k0 + 4 rg_b + s, s = 0..3
  const bool has_b = tid < nb;
  const int cg = nb / 4, c4 = (tid % cg) * 4, rg_b = has_b ? tid / cg : 0;
  const bool col_ok = has_b && b0 + c4 < a.B;
  const int64_t col = col_ok ? b0 + c4 : 0;  // (B % 4 == 0: a float4 of positions is wholly inside or outside)
  const int sw = (c4 >> 3) & 7;
  // W role: item idx = tid + i nt covers row a_m = idx >> 2 of the tile, k group a_rg = idx & 3 (16 contiguous bytes;
  // four neighbouring lanes read 64 contiguous bytes of one row)
  constexpr int A_ITEMS = MT * 128;
  constexpr int A_MAX = A_ITEMS / 64;  // items of a thread when the block is one wave

  const int kh = lane >> 5, j = lane & 31;
  const int jb = swizzle(wave * 32 + j);
  int ja[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) ja[mt] = swizzle(mt * 32 + j);

  int buf = 0;
  for (int l = 0; l < a.n_inputs; ++l) {
    const int K = a.n[l], koff = a.koff[l];
    const bool vec = a.vec0[l] != 0;  // block-uniform
    const float* src = a.rates[l] + (int64_t)t * K * a.B;
    v4f fa[A_MAX], fb[4];
    auto fetch = [&](int k0) {
      if (has_b) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {  // (ff_fetch: a row past K reads row K - 1, zeroed in the stash)
          const int k = k0 + 4 * rg_b + s;
          fb[s] = *reinterpret_cast<const v4f*>(src + (int64_t)(k < K ? k : K - 1) * a.B + col);
        }
      }
#pragma unroll
      for (int i = 0; i < A_MAX; ++i) {
        const int idx = tid + i * nt;
        if (idx < A_ITEMS) {
          // columns koff + k0 + 4 rg + e of W for k0 + 4 rg + e < K: mlp_w4's bounds argument with c_end = koff + K <= n_in
          // (vec0[l] also demands koff % 4 == 0, so that c % 4 == 0)
          const int c = koff + k0 + 4 * (idx & 3);
          fa[i] = vec ? mlp_w4<true>(L.w, L.n_in, L.n_out, m0 + (idx >> 2), c, koff + K)
                      : mlp_w4<false>(L.w, L.n_in, L.n_out, m0 + (idx >> 2), c, koff + K);
        }
      }
    };
    auto stash = [&](int b, int k0) {
      if (has_b) {  // 4x4 register transpose [s][column] -> [column][s]; rows >= K and columns outside the problem become 0
        v4f v[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) v[s] = (col_ok && k0 + 4 * rg_b + s < K) ? fb[s] : v4f{0.f, 0.f, 0.f, 0.f};
        float* dst = s_b + ((b * 4 + rg_b) * nb) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<v4f*>(dst + ((c4 + i) ^ sw) * 4) = v4f{v[0][i], v[1][i], v[2][i], v[3][i]};
      }
#pragma unroll
      for (int i = 0; i < A_MAX; ++i) {
        const int idx = tid + i * nt;
        if (idx < A_ITEMS) {
          const int am = idx >> 2;
          *reinterpret_cast<v4f*>(s_a + ((b * 4 + (idx & 3)) * 128 + swizzle(am)) * 4) = fa[i];
        }
      }
    };
    __syncthreads();  // the previous input's last slab has been consumed
    fetch(0);
    stash(buf, 0);
    __syncthreads();
    for (int k0 = 0; k0 < K; k0 += KT) {
      const bool more = k0 + KT < K;  // block-uniform
      if (more) fetch(k0 + KT);
#pragma unroll
      for (int g = 0; g < KT / 8; ++g) {
        const v4f bq = *reinterpret_cast<const v4f*>(s_b + ((buf * 4 + 2 * g + kh) * nb + jb) * 4);
        v4f aq[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) aq[mt] = *reinterpret_cast<const v4f*>(s_a + ((buf * 4 + 2 * g + kh) * 128 + ja[mt]) * 4);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[mt][s], bq[s], acc[mt], 0, 0, 0);
      }
      if (more) {
        stash(buf ^ 1, k0 + KT);  // the other buffer was last read one iteration ago (barrier below)
        __syncthreads();
        buf ^= 1;
      }
    }
  }
}

// Rows [m0, m0 + 32) of a layer >= 1 from the activations h of the layer before it (MTI = its 32-row tiles), operands
// straight from registers and from W in place (mlp_w4 states the bounds).
template <int MTI, bool VEC, int MAXT>
__device__ __forceinline__ v16f mlp_reg_tile(const v16f (&h)[MAXT], const MLPLayerArgs& L, int m0, int lane) {
  static_assert(MTI <= MAXT, "tile count");
  v16f acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  const int m = m0 + (lane & 31), kh = lane >> 5;
#pragma unroll
  for (int mi = 0; mi < MTI; ++mi) {
    v4f aq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) aq[q] = mlp_w4<VEC>(L.w, L.n_in, L.n_out, m, 32 * mi + 8 * q + 4 * kh, L.n_in);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[q][e], h[mi][4 * q + e], acc, 0, 0, 0);
    // (keeps the reads of the next 32 columns behind these MFMAs: hoisting all of a tile's reads costs > 100 registers
    // of addresses in the 4-byte form)
    __builtin_amdgcn_sched_barrier(0);
  }
  return acc;
}

// bias + activation of one 32-row tile in C/D layout; the last layer's rows are stored.  Rows >= n_out come out as
// act(0): finite, and multiplied by a zeroed A element in the next layer.
__device__ __forceinline__ v16f mlp_finish(v16f acc, const MLPLayerArgs& L, int m0, bool last, float* out, int64_t t,
                                           int64_t B, int64_t b, int lane) {
  const int row0 = m0 + 4 * (lane >> 5);
  v16f x;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = row0 + (r & 3) + 8 * (r >> 2);
    float bias = 0.0f;
    if (L.bias) {  // block-uniform; row clamped: the read lies in [bias, bias + n_out)
      const float v = L.bias[row < L.n_out ? row : L.n_out - 1];
      bias = row < L.n_out ? v : 0.0f;
    }
    x[r] = acc[r] + bias;
  }
  auto apply = [&](auto act_tag) {
    constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float d;
      x[r] = activate<ACT>(x[r], L.p0, L.p1, L.p2, L.p3, &d);
    }
  };
  switch (L.act) {  // block-uniform
    case RIAB_ACT_LINEAR: break;
    case RIAB_ACT_SIGMOID: apply(std::integral_constant<int, RIAB_ACT_SIGMOID>{}); break;
    case RIAB_ACT_RELU: apply(std::integral_constant<int, RIAB_ACT_RELU>{}); break;
    case RIAB_ACT_TANH: apply(std::integral_constant<int, RIAB_ACT_TANH>{}); break;
    case RIAB_ACT_RETANH: apply(std::integral_constant<int, RIAB_ACT_RETANH>{}); break;
    default: apply(std::integral_constant<int, RIAB_ACT_SOFTMAX>{}); break;
  }
  if (last && b < B) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + (r & 3) + 8 * (r >> 2);
      if (row < L.n_out) out[(t * L.n_out + row) * B + b] = x[r];
    }
  }
  return x;
}

// MAXT: the 32-row tiles of the widest activation the kernel carries (the hidden widths; the only layer's n_out, up to
// 128 rows a pass, when there is one layer).  Chosen by the host from the network's shape alone, so that a narrow network
// (the default 20-20) is not given the registers of a 128-wide one.
template <int MAXT>
__global__ __launch_bounds__(256) void mlp_kernel(const MLPArgs a) {
  extern __shared__ __align__(16) float mlp_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int nw = blockDim.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t b0 = (int64_t)blockIdx.x * (nw * 32);
  const int64_t b = b0 + wave * 32 + (lane & 31);
  const int t = blockIdx.z;
  const int n_layers = a.n_layers;
  v16f h[MAXT];  // (tiles past a layer's width are never read: the next layer walks ceil(n_in / 32) tiles)

  {  // layer 0.  More than one pass of 128 rows only when it is also the last layer (hidden widths are <= 128): those
     // passes keep nothing, so that no activation tile is carried around the streaming loop.
    const MLPLayerArgs& L = a.layer[0];
    const bool last = n_layers == 1;
    const int n_pass = last ? (L.n_out + 127) >> 7 : 1;
    for (int pass = 0; pass < n_pass; ++pass) {
      const int m0 = pass << 7, left = L.n_out - m0;
      v16f acc[MAXT];
      // (this choice of MT is restated for the host's record as mlp_pass_mt in riab_mlp_logic.h: change both together)
      if constexpr (MAXT == 4) {
        if (left > 64) mlp_first_layer<4, MAXT>(a, mlp_smem, m0, t, b0, nw, acc);
        else if (left > 32) mlp_first_layer<2, MAXT>(a, mlp_smem, m0, t, b0, nw, acc);
        else mlp_first_layer<1, MAXT>(a, mlp_smem, m0, t, b0, nw, acc);
      } else if constexpr (MAXT == 2) {
        if (left > 32) mlp_first_layer<2, MAXT>(a, mlp_smem, m0, t, b0, nw, acc);
        else mlp_first_layer<1, MAXT>(a, mlp_smem, m0, t, b0, nw, acc);
      } else {
        mlp_first_layer<1, MAXT>(a, mlp_smem, m0, t, b0, nw, acc);
      }
#pragma unroll
      for (int mt = 0; mt < MAXT; ++mt)
        if (32 * mt < left) acc[mt] = mlp_finish(acc[mt], L, m0 + 32 * mt, last, a.out, t, a.B, b, lane);
      if (!last) {
#pragma unroll
        for (int mt = 0; mt < MAXT; ++mt) h[mt] = acc[mt];
      }
    }
    if (last) return;
  }
  for (int l = 1; l < n_layers; ++l) {
    const MLPLayerArgs& L = a.layer[l];
    const bool last = l == n_layers - 1;
    const int mti = (L.n_in + 31) >> 5;  // 1..MAXT  (restated as mlp_mti in riab_mlp_logic.h: change both together)
    v16f hn[MAXT];
    for (int m0 = 0; m0 < L.n_out; m0 += 32) {  // (only the last layer has more than MAXT tiles)
      v16f acc;
      auto tile = [&](auto vec_tag) {
        constexpr bool VEC = decltype(vec_tag)::value;
        if constexpr (MAXT == 1) {
          acc = mlp_reg_tile<1, VEC, MAXT>(h, L, m0, lane);
        } else if constexpr (MAXT == 2) {
          if (mti == 1) acc = mlp_reg_tile<1, VEC, MAXT>(h, L, m0, lane);
          else acc = mlp_reg_tile<2, VEC, MAXT>(h, L, m0, lane);
        } else {
          switch (mti) {
            case 1: acc = mlp_reg_tile<1, VEC, MAXT>(h, L, m0, lane); break;
            case 2: acc = mlp_reg_tile<2, VEC, MAXT>(h, L, m0, lane); break;
            case 3: acc = mlp_reg_tile<3, VEC, MAXT>(h, L, m0, lane); break;
            default: acc = mlp_reg_tile<4, VEC, MAXT>(h, L, m0, lane); break;
          }
        }
      };
      if (L.vec) tile(std::true_type{});
      else tile(std::false_type{});
      acc = mlp_finish(acc, L, m0, last, a.out, t, a.B, b, lane);
      if (!last) {
        const int mo = m0 >> 5;  // block-uniform, < MAXT
#pragma unroll
        for (int i = 0; i < MAXT; ++i)
          if (mo == i) hn[i] = acc;
      }
    }
    if (!last) {
#pragma unroll
      for (int i = 0; i < MAXT; ++i) h[i] = hn[i];
    }
  }
}

// Workgroups of four waves (128 positions) when that grid already covers the chip; one wave (32 positions) otherwise, so
// that a one-row launch at 4096 agents is 128 workgroups, not 32.
int mlp_compute_units() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n <= 0) {
      (void)hipGetLastError();
      return 256;
    }
    cus = n;
  }
  return cus;
}

}  // namespace riab

using namespace riab;

extern "C" int riab_mlp_forward(const float* const* inputs, const int32_t* input_n, int32_t n_inputs,
                                const RiabMLPLayer* layers, int32_t n_layers, int64_t T, int64_t B, float* out,
                                riab_stream_t stream) {
  if (!inputs || !input_n || !layers) return RIAB_EINVAL;
  // the facts (entries past the limits are not read: mlp_validate refuses such a call by its counts) ...
  MLPFacts f = {};
  f.n_inputs = n_inputs;
  f.n_layers = n_layers;
  for (int l = 0; l < n_inputs && l < MLP_MAX_INPUTS; ++l)
    f.in[l] = MLPInputFacts{input_n[l], inputs[l] == nullptr, (unsigned)((uintptr_t)inputs[l] & 15)};
  for (int i = 0; i < n_layers && i < RIAB_MLP_MAX_LAYERS; ++i) {
    const RiabMLPLayer& q = layers[i];
    f.layer[i] = MLPLayerFacts{q.n_in, q.n_out, q.activation, q.w == nullptr, q.bias != nullptr, (unsigned)((uintptr_t)q.w & 15)};
  }
  f.T = T;
  f.B = B;
  f.out_null = out == nullptr;
  f.out_mod16 = (unsigned)((uintptr_t)out & 15);
  f.cus = mlp_compute_units();
  // ... the decision (riab_mlp_logic.h: every check and every choice of form is there) ...
  const MLPDecision d = mlp_decide(f);
  if (d.rc != RIAB_OK) return d.rc;
  // ... and its launch
  MLPArgs a;
  for (int l = 0; l < n_inputs; ++l) {
    a.rates[l] = inputs[l];
    a.n[l] = input_n[l];
    a.koff[l] = d.koff[l];
    a.vec0[l] = d.vec0[l];
  }
  for (int i = 0; i < n_layers; ++i) {
    const RiabMLPLayer& q = layers[i];
    MLPLayerArgs& L = a.layer[i];
    L.w = q.w;
    L.bias = q.bias;
    L.n_in = q.n_in;
    L.n_out = q.n_out;
    L.act = q.activation;
    L.vec = d.vec[i];
    L.p0 = q.act_params[0];
    L.p1 = q.act_params[1];
    L.p2 = q.act_params[2];
    L.p3 = q.act_params[3];
  }
  a.n_inputs = n_inputs;
  a.n_layers = n_layers;
  a.B = B;
  a.out = out;
  const dim3 grid(d.grid_x, 1, d.grid_z), block(64 * d.nw);
  if (d.maxt == 4) hipLaunchKernelGGL(mlp_kernel<4>, grid, block, d.lds_bytes, (hipStream_t)stream, a);
  else if (d.maxt == 2) hipLaunchKernelGGL(mlp_kernel<2>, grid, block, d.lds_bytes, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(mlp_kernel<1>, grid, block, d.lds_bytes, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
