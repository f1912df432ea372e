// FeedForwardLayer.get_state for gfx950 (reference Neurons.py:2797-2847, utils.activate
// utils.py:919-1026):
//
//     out[t][m][b] = act( sum_layers sum_k W_l[m][k] * I_l[t][k][b] + bias[m] )
//
// The one dense contraction on the path: a GEMM with M = n_out, K = n_in (summed over the
// input layers) and N = positions (agents x time rows, contiguous in memory for both the
// input rates and the output).  It runs on the fp32-input matrix cores,
// v_mfma_f32_32x32x2_f32: exact fp32 (a k-ordered fmaf chain), 64 FLOP/clk/SIMD.
//
// Workgroup = 4 waves; block tile = 32*MT outputs x 128 positions (MT = 4, 2 or 1 by layer width).  The main loop is the
// streamed GEMM core of riab_mfma_slab.h (fragment and LDS layout, swizzle, bounds and barriers are stated there), with
// W^T ([k][m], prepared on the host so that both operands are read with unit stride) as operand A.
// Epilogue: bias + activation (+ optional derivative) fused, 128-B row segments stored.
#include <type_traits>

#include "riab_act.h"   // activate<ACT>
#include "riab_device.h"
#include "riab_mfma_slab.h"

namespace riab {

constexpr int FF_MAX_LAYERS = 8;

struct FFArgs {
  const float* rates[FF_MAX_LAYERS];  // [T][n_in][B]
  const float* wt[FF_MAX_LAYERS];     // [n_in][Mp]  (W transposed, Mp = n_out padded to 32)
  int n_in[FF_MAX_LAYERS];
  int n_layers;
  const float* bias;  // [n_out]
  int n_out, Mp;
  int64_t B;
  int T;
  int act;
  float p0, p1, p2, p3;  // activation parameters
  float* out;            // [T][n_out][B]
  float* out_prime;      // or null
};

// 32 KB of LDS and < 170 registers per wave keep 3 workgroups (12 waves) on a CU, which is what hides
// the stash / barrier of one workgroup and the store epilogue of another behind the MFMAs of the third.
template <int MT>
__global__ __launch_bounds__(256) void ff_kernel(const FFArgs a) {
  __shared__ __align__(16) SlabTiles<MT> lds;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t b0 = (int64_t)blockIdx.x * NB;  // first agent of the block's position tile
  const int m0 = blockIdx.y * (MT * 32);        // first output of the block
  const int t = blockIdx.z;
  // bias rows of this block, read back through LDS in the epilogue: a global load there would make
  // every s_waitcnt vmcnt also wait for the stores issued before it (one write round trip per row)
  __shared__ float s_bias[MT * 32];
  if (tid < MT * 32) s_bias[tid] = m0 + tid < a.n_out ? a.bias[m0 + tid] : 0.0f;
  v16f acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) zero_acc(acc[i]);

  const SlabRole<MT> role(lds, tid, wave);
  const Frag<MT> fr(lane, wave);
  const bool is_b = role.is_b;
  const SlabMask mask = {is_b ? (b0 + role.c4 < a.B) : role.a_quad_ok(m0, a.Mp), 4};
  const int64_t col = mask.col_ok ? (is_b ? b0 + role.c4 : (int64_t)m0 + role.c4) : 0;
  const int64_t ld = is_b ? a.B : (int64_t)a.Mp;
  int buf = 0;
  for (int l = 0; l < a.n_layers; ++l) {
    const int K = a.n_in[l];
    const float* src = is_b ? a.rates[l] + (int64_t)t * K * a.B : a.wt[l];
    __syncthreads();  // the previous layer's last slab has been consumed
    contract_population(lds, role, fr, buf, K, mask, acc, [&](int kbase) { return fetch_f32(src, ld, col, K, kbase); });
  }
  // ---- epilogue: bias + activation, in the C/D layout of riab_mfma_slab.h
  const int64_t b = b0 + wave * 32 + (lane & 31);
  if (b < a.B) {
    const int row0 = 4 * (lane >> 5);
    const int64_t off0 = ((int64_t)t * a.n_out + m0 + row0) * a.B + b;
    const int rows_left = a.n_out - m0 - row0;  // rows ml (relative to row0) < rows_left are real outputs
    auto store_tiles = [&](auto act_tag, auto prime_tag) {
      constexpr int ACT = decltype(act_tag)::value;
      constexpr bool PRIME = decltype(prime_tag)::value;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ml = mt * 32 + (r & 3) + 8 * (r >> 2);  // compile-time
          if (ml < rows_left) {
            float d;
            const float f = activate<ACT>(acc[mt][r] + s_bias[ml + row0], a.p0, a.p1, a.p2, a.p3, &d);
            a.out[off0 + (int64_t)ml * a.B] = f;
            if (PRIME) a.out_prime[off0 + (int64_t)ml * a.B] = d;
          }
        }
      }
    };
    auto with_act = [&](auto act_tag) {
      if (a.out_prime) store_tiles(act_tag, std::true_type{});
      else store_tiles(act_tag, std::false_type{});
    };
    switch (a.act) {  // block-uniform
      case RIAB_ACT_LINEAR: with_act(std::integral_constant<int, RIAB_ACT_LINEAR>{}); break;
      case RIAB_ACT_SIGMOID: with_act(std::integral_constant<int, RIAB_ACT_SIGMOID>{}); break;
      case RIAB_ACT_RELU: with_act(std::integral_constant<int, RIAB_ACT_RELU>{}); break;
      case RIAB_ACT_TANH: with_act(std::integral_constant<int, RIAB_ACT_TANH>{}); break;
      case RIAB_ACT_RETANH: with_act(std::integral_constant<int, RIAB_ACT_RETANH>{}); break;
      default: with_act(std::integral_constant<int, RIAB_ACT_SOFTMAX>{}); break;
    }
  }
}

}  // namespace riab

using namespace riab;

extern "C" int riab_feedforward(const RiabFFInput* inputs, int32_t n_inputs, const float* bias, int32_t n_out,
                                int64_t T, int64_t B, int32_t activation, const float* act_params, float* out,
                                float* out_prime, riab_stream_t stream) {
  if (!inputs || n_inputs <= 0 || !bias || n_out <= 0 || T <= 0 || B <= 0 || !out || !act_params) return RIAB_EINVAL;
  if (n_inputs > FF_MAX_LAYERS) return RIAB_ETOOBIG;
  if (activation < RIAB_ACT_LINEAR || activation > RIAB_ACT_SOFTMAX) return RIAB_EINVAL;
  if (B % 4 != 0 || T > 65535) return B % 4 ? RIAB_EALIGN : RIAB_ETOOBIG;
  FFArgs a;
  a.Mp = (n_out + 31) / 32 * 32;
  for (int l = 0; l < n_inputs; ++l) {
    if (!inputs[l].rates || !inputs[l].wt || inputs[l].n_in <= 0) return RIAB_EINVAL;
    if ((((uintptr_t)inputs[l].rates | (uintptr_t)inputs[l].wt) & 15)) return RIAB_EALIGN;
    a.rates[l] = inputs[l].rates;
    a.wt[l] = inputs[l].wt;
    a.n_in[l] = inputs[l].n_in;
  }
  a.n_layers = n_inputs;
  a.bias = bias;
  a.n_out = n_out;
  a.B = B;
  a.T = (int)T;
  a.act = activation;
  a.p0 = act_params[0];
  a.p1 = act_params[1];
  a.p2 = act_params[2];
  a.p3 = act_params[3];
  a.out = out;
  a.out_prime = out_prime;
  // outputs per block: 128 (4 MFMA row tiles), 64 or 32 for narrow layers
  const int mt = a.Mp >= 128 ? 4 : (a.Mp >= 64 ? 2 : 1);
  const dim3 grid((unsigned)((B + NB - 1) / NB), (unsigned)((a.Mp + mt * 32 - 1) / (mt * 32)), (unsigned)T);
  if (mt == 4) hipLaunchKernelGGL(ff_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else if (mt == 2) hipLaunchKernelGGL(ff_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(ff_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
