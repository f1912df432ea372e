// Continuous-time TD(lambda) learning for gfx950: contribs.ValueNeuron / contribs.SuccessorFeatures (reference
// contribs/ValueNeuron.py:59-113).  ONE learner fed by the whole batch:
//
//     update():          dVdt = (V - V_last) / dt;   e_l = dt * phi_l + (1 - dt / tau_e) * e_l
//     update_weights(r): td   = r + dVdt - V / tau
//                        W_l += dt * eta / B * sum_{b<B} (td * prime)[:, b] (x) e_l[:, b]  -  eta * dt * L2 * W_l
//
// The hot path is the batch-long reduction G[i][j] = sum_b g[i][b] * e_l[j][b], g = td * prime: a GEMM with M = n
// (padded to 32), N = n_in and K = the batch, both operands stored [row][Bp], so K is the unit-stride axis of both.  It
// runs on v_mfma_f32_32x32x2_f32 (exact fp32; fragment layout in the header of riab_ff.hip).
//
// td_grad_kernel: workgroup = 4 waves = 128 rows of e_l (wave w owns rows [32w, 32w+32) and all MT 32-row tiles of g) x
// one chunk of the batch, walked in slabs of 32 lanes.  A slab of e_l is fetched by coalesced 16-B loads (8 threads = one
// 128-B row segment), a slab of g is computed on the fly from r, V, dVdt and prime, both are staged in LDS with a row
// pitch of 36 floats (16-B fragment reads of 16 consecutive rows touch 64 different banks); the loads of slab i+1 are in
// flight while slab i feeds the MFMAs.  The order of the k-steps inside a slab is free as long as both operands agree:
// lanes 0-31 take lanes 8q..8q+3 of the batch, lanes 32-63 take 8q+4..8q+7, so a fragment is ONE ds_read_b128.
// FUSE: the trace update rides in the same pass (phi read, e read, new e stored and fed to the MFMAs): the trace is
// read once per step.  Lanes b >= B are zeroed in LDS on both sides: padded lanes contribute nothing, whatever they hold.
// The chunk's partial G goes to a workspace; td_combine_kernel adds the partials in a fixed order (no float atomics: a
// run is bit-identical to the next) and applies the update to W^T [n_in][Mp], the layout riab_feedforward reads.
//
// riab_td_learn_step: a whole `learn(reward); reset(lanes = mask)` behind the forward pass in TWO launches, for the step
// plan's learner stage.  DVDT: the gradient pass works dV/dt out from V and V_last on the fly (the workgroups that store
// the TD error store it too; V_last is read by every workgroup of the grid, so it is not written there).
// td_finish_kernel: td_combine_kernel's blocks, and behind them blocks that copy V to V_last and zero the columns of the
// masked lanes.  Stream order is all the two launches rely on.
#include "riab_device.h"
#include "riab_launch.h"

namespace riab {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int TD_MAX_LAYERS = 8;
constexpr int TD_MAX_ROWS = 8;
constexpr int TD_JB = 128;      // rows of e_l per workgroup
constexpr int TD_KB = 32;       // lanes of the batch per slab
constexpr int TD_LD = 36;       // LDS row pitch
constexpr int TD_MAX_CHUNKS = 64;
constexpr int TD_TARGET_WGS = 512;  // two workgroups per compute unit

struct TDLayerArgs {
  const float* rates;  // [n_in][Bp]
  float* trace;        // [n_in][Bp]
  float* wt;           // [n_in][Mp]
  float* partial;      // [chunk][n][n_in]
  int n_in;
  int jb0;             // first 128-row block of this layer in grid.x
};

struct TDGradArgs {
  TDLayerArgs layer[TD_MAX_LAYERS];
  int n_layers;
  const void* reward;
  int reward_f64;
  int64_t r_ld_n, r_ld_b;
  const float *v, *dvdt, *prime;
  float* td;
  const float* v_last;  // DVDT: dvdt_out = (v - v_last) / dt is worked out here ...
  float* dvdt_out;      // ... and stored by the workgroups that store td
  float dt;
  int n;
  int64_t B, Bp;
  int slabs_per_chunk;
  float tau, c_phi, c_e;
};

struct TDCombineArgs {
  TDLayerArgs layer[TD_MAX_LAYERS];
  int n, Mp, n_chunks;
  float scale, decay;
};

// td_finish_kernel: the combine blocks [0, n_combine) = (cx, n, layers) flattened, then the blocks of the [n][Bp] rows
// (V -> V_last, masked columns zeroed), then — with a mask — those of every layer's trace from tb0[l] on
struct TDFinishArgs {
  TDCombineArgs c;
  int cx, n_combine;
  int tb0[TD_MAX_LAYERS + 1];
  float* v;  // zeroed in the masked columns when zero_v (the caller's row is not a history row)
  float *v_last, *dvdt, *td;
  const uint8_t* mask;
  int zero_v;
  int64_t B, Bp;
};

struct TDTailArgs {
  TDLayerArgs layer[TD_MAX_LAYERS];
  int64_t Bp;
  float c_phi, c_e;
};

struct TDResetArgs {
  float* rows[TD_MAX_LAYERS + TD_MAX_ROWS];
  int n_rows[TD_MAX_LAYERS + TD_MAX_ROWS];
  const uint8_t* mask;
  int64_t B, Bp;
};

// e = dt * phi + (1 - dt / tau_e) * e, every operation rounded on its own: the stand-alone kernel and the fused pass of
// td_grad_kernel give the same bits
__device__ __forceinline__ v4f trace_next(v4f phi, v4f e, float c_phi, float c_e) {
#pragma clang fp contract(off)
  const v4f a = c_phi * phi;
  const v4f b = c_e * e;
  return a + b;
}

// dVdt = (V - V_last) / dt and td = r + dVdt - V / tau: td_dvdt_kernel, td_grad_kernel and its DVDT form give the same bits
__device__ __forceinline__ v4f dvdt_of(v4f v, v4f v_last, float dt) {
#pragma clang fp contract(off)
  return (v - v_last) / dt;
}
__device__ __forceinline__ float td_of(float r, float dvdt, float v, float tau) {
#pragma clang fp contract(off)
  return (r + dvdt) - v / tau;
}

__device__ __forceinline__ float reward_at(const TDGradArgs& a, int i, int64_t b) {
  const int64_t idx = (int64_t)i * a.r_ld_n + b * a.r_ld_b;
  return a.reward_f64 ? (float)static_cast<const double*>(a.reward)[idx] : static_cast<const float*>(a.reward)[idx];
}

struct TDSlab {
  v4f e[4], phi[4];
};

template <int MT, bool FUSE, bool DVDT>
__global__ __launch_bounds__(256) void td_grad_kernel(const TDGradArgs a) {
  __shared__ __align__(16) float s_e[TD_JB][TD_LD];
  __shared__ __align__(16) float s_g[MT * 32][TD_LD];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int l = 0;
  while (l + 1 < a.n_layers && (int)blockIdx.x >= a.layer[l + 1].jb0) ++l;  // block-uniform
  const float* const rates = a.layer[l].rates;
  float* const trace = a.layer[l].trace;
  const int n_in = a.layer[l].n_in;
  const int j0 = ((int)blockIdx.x - a.layer[l].jb0) * TD_JB;
  const int m0 = blockIdx.z * (MT * 32);
  const int64_t bc0 = (int64_t)blockIdx.y * a.slabs_per_chunk * TD_KB;
  const int64_t bc_end = bc0 + (int64_t)a.slabs_per_chunk * TD_KB;
  const int64_t bc1 = bc_end < a.Bp ? bc_end : a.Bp;
  const bool writes_td = blockIdx.x == 0;  // one workgroup per (chunk, row group) stores the TD error
  const int g_rows = a.n - m0 < MT * 32 ? a.n - m0 : MT * 32;

  for (int idx = tid; idx < MT * 32 * TD_LD; idx += 256) (&s_g[0][0])[idx] = 0.0f;  // rows >= n stay zero
  v16f acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

  // fetch role: rows r0 + 32 s (s = 0..3) x 4 consecutive lanes of the batch (Bp is a multiple of 4: a quad is wholly
  // inside or outside the arrays)
  const int c4 = (tid & 7) * 4, r0 = tid >> 3;
  auto fetch = [&](int64_t b0) {
    TDSlab f;
    const int64_t b = b0 + c4;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int jr = j0 + r0 + 32 * s;
      const bool ok = b < a.Bp && jr < n_in;
      const int64_t off = ok ? (int64_t)jr * a.Bp + b : 0;
      f.e[s] = *reinterpret_cast<const v4f*>(trace + off);
      if (FUSE) f.phi[s] = *reinterpret_cast<const v4f*>(rates + off);
    }
    return f;
  };
  // new trace to memory (FUSE) and, with the padded lanes zeroed, to LDS
  auto stash = [&](const TDSlab& f, int64_t b0) {
    const int64_t b = b0 + c4;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int jr = j0 + r0 + 32 * s;
      const bool ok = b < a.Bp && jr < n_in;
      v4f e = f.e[s];
      if (FUSE) {
        e = trace_next(f.phi[s], e, a.c_phi, a.c_e);
        if (ok && blockIdx.z == 0) *reinterpret_cast<v4f*>(trace + (int64_t)jr * a.Bp + b) = e;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) e[k] = (ok && b + k < a.B) ? e[k] : 0.0f;
      *reinterpret_cast<v4f*>(&s_e[r0 + 32 * s][c4]) = e;
    }
  };
  // g = td * prime of this slab, computed on the fly
  auto stash_g = [&](int64_t b0) {
    for (int idx = tid; idx < g_rows * (TD_KB / 4); idx += 256) {
      const int il = idx >> 3, cc = (idx & 7) * 4;
      const int i = m0 + il;
      const int64_t b = b0 + cc;
      v4f g = v4f{0.f, 0.f, 0.f, 0.f};
      if (b < a.Bp) {
        const int64_t off = (int64_t)i * a.Bp + b;
        const v4f v = *reinterpret_cast<const v4f*>(a.v + off);
        v4f dv;
        if (DVDT) {
          dv = dvdt_of(v, *reinterpret_cast<const v4f*>(a.v_last + off), a.dt);
          if (writes_td) *reinterpret_cast<v4f*>(a.dvdt_out + off) = dv;
        } else {
          dv = *reinterpret_cast<const v4f*>(a.dvdt + off);
        }
        const v4f pr = *reinterpret_cast<const v4f*>(a.prime + off);
        v4f td = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (b + k < a.B) {
            td[k] = td_of(reward_at(a, i, b + k), dv[k], v[k], a.tau);
            g[k] = td[k] * pr[k];
          }
        }
        if (writes_td) *reinterpret_cast<v4f*>(a.td + off) = td;
      }
      *reinterpret_cast<v4f*>(&s_g[il][cc]) = g;
    }
  };

  const int kh = lane >> 5, j = lane & 31;
  TDSlab cur = fetch(bc0);
  for (int64_t b0 = bc0; b0 < bc1; b0 += TD_KB) {
    __syncthreads();  // the previous slab has been consumed (first pass: s_g has been cleared)
    stash(cur, b0);
    stash_g(b0);
    __syncthreads();
    if (b0 + TD_KB < bc1) cur = fetch(b0 + TD_KB);  // block-uniform; in flight under the MFMAs
#pragma unroll
    for (int q = 0; q < TD_KB / 8; ++q) {
      const v4f bq = *reinterpret_cast<const v4f*>(&s_e[wave * 32 + j][8 * q + 4 * kh]);
      v4f aq[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) aq[mt] = *reinterpret_cast<const v4f*>(&s_g[mt * 32 + j][8 * q + 4 * kh]);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[mt][s], bq[s], acc[mt], 0, 0, 0);
    }
  }
  // ---- the chunk's partial sums: C/D layout col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
  const int jj = j0 + wave * 32 + j;
  if (jj < n_in) {
    float* const out = a.layer[l].partial + (int64_t)blockIdx.y * a.n * n_in + jj;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = m0 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (i < a.n) out[(int64_t)i * n_in] = acc[mt][r];
      }
    }
  }
}

// W^T[j][i] += scale * sum_chunks partial[c][i][j] - decay * W^T[j][i]; grid (n_in / 64, n, layers).  Workgroup = 64
// inputs x 4 chunk groups: thread (j, q) adds the chunks q, q + 4, q + 8, ... in that order (the loads do not depend on
// the sum: eight are in flight), then the four group sums are added in the order 0, 1, 2, 3 — a fixed order, whatever
// the machine does.
__device__ __forceinline__ void td_combine_block(const TDCombineArgs& a, int bx, int by, int bz) {
  __shared__ float s_part[4][64];
  const TDLayerArgs& L = a.layer[bz];
  const int jl = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int jj = bx * 64 + jl, i = by;
  float g = 0.0f;
  if (jj < L.n_in) {
    const float* p = L.partial + (int64_t)i * L.n_in + jj;
    const int64_t stride = (int64_t)a.n * L.n_in;
#pragma unroll 8
    for (int c = q; c < a.n_chunks; c += 4) g += p[c * stride];
  }
  s_part[q][jl] = g;
  __syncthreads();
  if (q == 0 && jj < L.n_in) {
    const float sum = ((s_part[0][jl] + s_part[1][jl]) + s_part[2][jl]) + s_part[3][jl];
    float* const w = L.wt + (int64_t)jj * a.Mp + i;
    const float w0 = *w;
    *w = w0 + (a.scale * sum - a.decay * w0);
  }
}
__global__ __launch_bounds__(256) void td_combine_kernel(const TDCombineArgs a) {
  td_combine_block(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

// which of the quad's lanes b .. b + 3 are reset: b + k < B with mask[b + k] != 0
__device__ __forceinline__ bool td_quad_hits(const uint8_t* mask, int64_t b, int64_t B, bool hit[4]) {
  bool any = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    hit[k] = b + k < B && mask[b + k] != 0;
    any |= hit[k];
  }
  return any;
}
__device__ __forceinline__ void td_zero_hits(float* rows, int64_t q, const bool hit[4]) {
  v4f* const p = reinterpret_cast<v4f*>(rows) + q;
  v4f x = *p;
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = hit[k] ? 0.0f : x[k];
  *p = x;
}

// The second launch of riab_td_learn_step: td_combine_kernel's blocks (same sums, same order), then V_last = V and
// ValueNeuron.reset(lanes = mask) — only quads with a masked lane are rewritten, as td_reset_kernel does.
__global__ __launch_bounds__(256) void td_finish_kernel(const TDFinishArgs a) {
  const int blk = blockIdx.x;  // block-uniform branches throughout
  if (blk < a.n_combine) {
    const int per_layer = a.cx * a.c.n;
    const int bz = blk / per_layer, rest = blk - bz * per_layer;
    td_combine_block(a.c, rest % a.cx, rest / a.cx, bz);
    return;
  }
  const int tb = blk - a.n_combine;
  const int64_t qpr = a.Bp / 4;
  if (tb < a.tb0[0]) {  // the [n][Bp] rows
    const int64_t q = (int64_t)tb * 256 + threadIdx.x;
    if (q >= (int64_t)a.c.n * qpr) return;
    bool hit[4] = {false, false, false, false};
    const bool any = a.mask && td_quad_hits(a.mask, (q % qpr) * 4, a.B, hit);
    v4f x = reinterpret_cast<const v4f*>(a.v)[q];
    if (any) {
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = hit[k] ? 0.0f : x[k];
      if (a.zero_v) reinterpret_cast<v4f*>(a.v)[q] = x;
      td_zero_hits(a.dvdt, q, hit);
      td_zero_hits(a.td, q, hit);
    }
    reinterpret_cast<v4f*>(a.v_last)[q] = x;
    return;
  }
  int l = 0;  // a trace (blocks exist only with a mask)
  while (tb >= a.tb0[l + 1]) ++l;
  const int64_t q = (int64_t)(tb - a.tb0[l]) * 256 + threadIdx.x;
  if (q >= (int64_t)a.c.layer[l].n_in * qpr) return;
  bool hit[4];
  if (td_quad_hits(a.mask, (q % qpr) * 4, a.B, hit)) td_zero_hits(a.c.layer[l].trace, q, hit);
}

// dVdt = (V - V_last) / dt; V_last = V
__global__ __launch_bounds__(256) void td_dvdt_kernel(const float* v, float* v_last, float* dvdt, int64_t quads, float dt) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= quads) return;
  const v4f x = reinterpret_cast<const v4f*>(v)[q];
  const v4f x0 = reinterpret_cast<const v4f*>(v_last)[q];
  reinterpret_cast<v4f*>(dvdt)[q] = dvdt_of(x, x0, dt);
  reinterpret_cast<v4f*>(v_last)[q] = x;
}

// the stand-alone trace update; grid (quads of the widest layer, layers)
__global__ __launch_bounds__(256) void td_trace_kernel(const TDTailArgs a) {
  const TDLayerArgs& L = a.layer[blockIdx.y];
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (int64_t)L.n_in * a.Bp / 4) return;
  const v4f phi = reinterpret_cast<const v4f*>(L.rates)[q];
  v4f* const e = reinterpret_cast<v4f*>(L.trace) + q;
  *e = trace_next(phi, *e, a.c_phi, a.c_e);
}

// zero the columns b < B with mask[b] != 0 (no mask: all of them) of every array; grid (quads of the tallest, arrays)
__global__ __launch_bounds__(256) void td_reset_kernel(const TDResetArgs a) {
  float* const rows = a.rows[blockIdx.y];
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t qpr = a.Bp / 4;
  if (q >= (int64_t)a.n_rows[blockIdx.y] * qpr) return;
  const int64_t b = (q % qpr) * 4;
  bool hit[4], any = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    hit[k] = b + k < a.B && (!a.mask || a.mask[b + k] != 0);
    any |= hit[k];
  }
  if (!any) return;
  v4f* const p = reinterpret_cast<v4f*>(rows) + q;
  v4f x = *p;
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = hit[k] ? 0.0f : x[k];
  *p = x;
}

// ---- host side -------------------------------------------------------------------------------------------------
int td_check(const RiabTDParams* p, const RiabTDLayer* layers, int32_t n_layers) {
  if (!p || !layers || n_layers <= 0) return RIAB_EINVAL;
  if (n_layers > TD_MAX_LAYERS) return RIAB_ETOOBIG;
  if (p->n <= 0 || p->B <= 0 || p->Bp < p->B || p->Mp % 32 != 0 || p->n > p->Mp) return RIAB_EINVAL;
  if (!(p->dt > 0.0f) || !(p->tau > 0.0f) || !(p->tau_e >= 0.0f)) return RIAB_EINVAL;
  if (p->Bp % 4 != 0) return RIAB_EALIGN;
  if (p->n > 65535) return RIAB_ETOOBIG;
  for (int l = 0; l < n_layers; ++l) {
    if (!layers[l].rates || !layers[l].trace || !layers[l].wt || layers[l].n_in <= 0) return RIAB_EINVAL;
    if ((((uintptr_t)layers[l].rates | (uintptr_t)layers[l].trace | (uintptr_t)layers[l].wt) & 15)) return RIAB_EALIGN;
  }
  return RIAB_OK;
}

// how the batch is split: chunks of `slabs` 32-lane slabs each, so that about TD_TARGET_WGS workgroups exist
static int td_chunks(const RiabTDParams* p, const RiabTDLayer* layers, int32_t n_layers, int* slabs) {
  int64_t blocks = 0;
  for (int l = 0; l < n_layers; ++l) blocks += (layers[l].n_in + TD_JB - 1) / TD_JB;
  const int64_t n_slabs = (p->Bp + TD_KB - 1) / TD_KB;
  int64_t want = TD_TARGET_WGS / blocks;
  want = want < 1 ? 1 : (want > TD_MAX_CHUNKS ? TD_MAX_CHUNKS : want);
  want = want > n_slabs ? n_slabs : want;
  *slabs = (int)((n_slabs + want - 1) / want);
  return (int)((n_slabs + *slabs - 1) / *slabs);
}

static void td_trace_coefficients(const RiabTDParams* p, float* c_phi, float* c_e) {
  if (p->tau_e == 0.0f) {
    *c_phi = 1.0f;
    *c_e = 0.0f;
  } else {
    *c_phi = p->dt;
    *c_e = (float)(1.0 - (double)p->dt / (double)p->tau_e);
  }
}

static void td_launch_trace(const RiabTDParams* p, const RiabTDLayer* layers, int32_t n_layers, hipStream_t stream) {
  TDTailArgs t = {};
  int64_t quads = 0;
  for (int l = 0; l < n_layers; ++l) {
    t.layer[l].rates = layers[l].rates;
    t.layer[l].trace = layers[l].trace;
    t.layer[l].n_in = layers[l].n_in;
    const int64_t q = (int64_t)layers[l].n_in * p->Bp / 4;
    quads = q > quads ? q : quads;
  }
  t.Bp = p->Bp;
  td_trace_coefficients(p, &t.c_phi, &t.c_e);
  hipLaunchKernelGGL(td_trace_kernel, dim3((unsigned)((quads + 255) / 256), (unsigned)n_layers), dim3(256), 0, stream, t);
}

template <int MT, bool DVDT>
static void td_launch_grad(const TDGradArgs& g, dim3 grid, bool fuse, hipStream_t stream) {
  if (fuse) hipLaunchKernelGGL((td_grad_kernel<MT, true, DVDT>), grid, dim3(256), 0, stream, g);
  else hipLaunchKernelGGL((td_grad_kernel<MT, false, DVDT>), grid, dim3(256), 0, stream, g);
}
template <int MT>
static void td_launch_grad(const TDGradArgs& g, dim3 grid, bool fuse, hipStream_t stream) {
  if (g.v_last) td_launch_grad<MT, true>(g, grid, fuse, stream);
  else td_launch_grad<MT, false>(g, grid, fuse, stream);
}

// The checks riab_td_update and riab_td_learn_step share, [the stand-alone trace kernel] and the gradient launch;
// `c`: the arguments of the combine that follows.  v_last != null: dvdt is written here (the DVDT form), not read.
static int td_gradient(const RiabTDParams* p, const RiabTDLayer* layers, int32_t n_layers, const void* reward,
                       int32_t reward_f64, int64_t reward_ld_n, int64_t reward_ld_b, const float* v, const float* v_last,
                       float* dvdt, const float* prime, float* td, int32_t fuse_trace, float* workspace,
                       int64_t workspace_floats, hipStream_t stream, TDCombineArgs& c, int* widest_out) {
  const int rc = td_check(p, layers, n_layers);
  if (rc != RIAB_OK) return rc;
  if (!reward || !v || !dvdt || !prime || !td || !workspace || reward_ld_n < 0 || reward_ld_b < 0) return RIAB_EINVAL;
  if ((((uintptr_t)v | (uintptr_t)v_last | (uintptr_t)dvdt | (uintptr_t)prime | (uintptr_t)td | (uintptr_t)workspace) & 15))
    return RIAB_EALIGN;
  if (((uintptr_t)reward & (reward_f64 ? 7 : 3))) return RIAB_EALIGN;
  if (workspace_floats < riab_td_workspace(p, layers, n_layers)) return RIAB_EINVAL;
  TDGradArgs g = {};
  c = {};
  const int n_chunks = td_chunks(p, layers, n_layers, &g.slabs_per_chunk);
  int jb = 0, widest = 0;
  float* part = workspace;
  for (int l = 0; l < n_layers; ++l) {
    TDLayerArgs& L = g.layer[l];
    L.rates = layers[l].rates;
    L.trace = layers[l].trace;
    L.wt = layers[l].wt;
    L.partial = part;
    L.n_in = layers[l].n_in;
    L.jb0 = jb;
    c.layer[l] = L;
    jb += (layers[l].n_in + TD_JB - 1) / TD_JB;
    part += (int64_t)n_chunks * p->n * layers[l].n_in;
    widest = layers[l].n_in > widest ? layers[l].n_in : widest;
  }
  g.n_layers = n_layers;
  g.reward = reward;
  g.reward_f64 = reward_f64;
  g.r_ld_n = reward_ld_n;
  g.r_ld_b = reward_ld_b;
  g.v = v;
  g.dvdt = dvdt;
  g.prime = prime;
  g.td = td;
  g.v_last = v_last;
  g.dvdt_out = dvdt;
  g.dt = p->dt;
  g.n = p->n;
  g.B = p->B;
  g.Bp = p->Bp;
  g.tau = p->tau;
  td_trace_coefficients(p, &g.c_phi, &g.c_e);
  // all row tiles of g in one workgroup (up to 8: 128 accumulator registers); wider learners take several row groups,
  // and then the trace is updated by its own kernel first (two groups must not both rewrite it)
  const int tiles = p->Mp / 32 < (p->n + 31) / 32 ? p->Mp / 32 : (p->n + 31) / 32;
  const int mt = tiles <= 1 ? 1 : (tiles <= 2 ? 2 : (tiles <= 4 ? 4 : 8));
  const int groups = (tiles + mt - 1) / mt;
  bool fuse = fuse_trace != 0;
  if (fuse && groups > 1) {
    td_launch_trace(p, layers, n_layers, stream);
    fuse = false;
  }
  const dim3 grid((unsigned)jb, (unsigned)n_chunks, (unsigned)groups);
  if (mt == 1) td_launch_grad<1>(g, grid, fuse, stream);
  else if (mt == 2) td_launch_grad<2>(g, grid, fuse, stream);
  else if (mt == 4) td_launch_grad<4>(g, grid, fuse, stream);
  else td_launch_grad<8>(g, grid, fuse, stream);
  c.n = p->n;
  c.Mp = p->Mp;
  c.n_chunks = n_chunks;
  c.scale = (float)((double)p->dt * (double)p->eta / (double)p->B);
  c.decay = (float)((double)p->eta * (double)p->dt * (double)p->L2);
  *widest_out = widest;
  return RIAB_OK;
}

}  // namespace riab

using namespace riab;

extern "C" int riab_td_forward_tail(const RiabTDParams* p, const RiabTDLayer* layers, int32_t n_layers, const float* v,
                                    float* v_last, float* dvdt, int32_t with_trace, riab_stream_t stream) {
  const int rc = td_check(p, layers, n_layers);
  if (rc != RIAB_OK) return rc;
  if ((v || dvdt) && (!v || !dvdt || !v_last)) return RIAB_EINVAL;
  if ((((uintptr_t)v | (uintptr_t)v_last | (uintptr_t)dvdt) & 15)) return RIAB_EALIGN;
  if (v) {
    const int64_t quads = (int64_t)p->n * p->Bp / 4;
    hipLaunchKernelGGL(td_dvdt_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v, v_last,
                       dvdt, quads, p->dt);
  }
  if (with_trace) td_launch_trace(p, layers, n_layers, (hipStream_t)stream);
  return (int)hipGetLastError();
}

extern "C" int64_t riab_td_workspace(const RiabTDParams* p, const RiabTDLayer* layers, int32_t n_layers) {
  if (!p || !layers || n_layers <= 0 || n_layers > TD_MAX_LAYERS || p->n <= 0 || p->Bp <= 0) return RIAB_EINVAL;
  int64_t n_in = 0;
  for (int l = 0; l < n_layers; ++l) {
    if (layers[l].n_in <= 0) return RIAB_EINVAL;
    n_in += layers[l].n_in;
  }
  int slabs;
  return (int64_t)td_chunks(p, layers, n_layers, &slabs) * p->n * n_in;
}

extern "C" int riab_td_update(const RiabTDParams* p, const RiabTDLayer* layers, int32_t n_layers, const void* reward,
                              int32_t reward_f64, int64_t reward_ld_n, int64_t reward_ld_b, const float* v,
                              const float* dvdt, const float* prime, float* td, int32_t fuse_trace, float* workspace,
                              int64_t workspace_floats, riab_stream_t stream) {
  TDCombineArgs c;
  int widest;
  const int rc = td_gradient(p, layers, n_layers, reward, reward_f64, reward_ld_n, reward_ld_b, v, nullptr,
                             const_cast<float*>(dvdt), prime, td, fuse_trace, workspace, workspace_floats, (hipStream_t)stream, c,
                             &widest);
  if (rc != RIAB_OK) return rc;
  hipLaunchKernelGGL(td_combine_kernel, dim3((unsigned)((widest + 63) / 64), (unsigned)p->n, (unsigned)n_layers), dim3(256),
                     0, (hipStream_t)stream, c);
  return (int)hipGetLastError();
}

extern "C" int riab_td_learn_step(const RiabTDParams* p, const RiabTDLayer* layers, int32_t n_layers, const void* reward,
                                  int32_t reward_f64, int64_t reward_ld_n, int64_t reward_ld_b, float* v, float* v_last,
                                  float* dvdt, const float* prime, float* td, const uint8_t* mask, int32_t zero_v,
                                  float* workspace, int64_t workspace_floats, riab_stream_t stream) {
  if (!v_last) return RIAB_EINVAL;
  // (what the finish launch's flat grid holds is checked before the gradient is launched)
  int rc = td_check(p, layers, n_layers);
  if (rc != RIAB_OK) return rc;
  TDFinishArgs f = {};
  int widest = 0;
  for (int l = 0; l < n_layers; ++l) widest = layers[l].n_in > widest ? layers[l].n_in : widest;
  f.cx = (widest + 63) / 64;
  const int64_t qpr = p->Bp / 4;
  int64_t blocks = (int64_t)f.cx * p->n * n_layers;
  if (blocks > INT32_MAX / 2) return RIAB_ETOOBIG;
  f.n_combine = (int)blocks;
  int64_t tb = (p->n * qpr + 255) / 256;
  for (int l = 0; l <= n_layers; ++l) {
    if (blocks + tb > INT32_MAX / 2) return RIAB_ETOOBIG;
    f.tb0[l] = (int)tb;
    if (l < n_layers && mask) tb += (layers[l].n_in * qpr + 255) / 256;
  }
  rc = td_gradient(p, layers, n_layers, reward, reward_f64, reward_ld_n, reward_ld_b, v, v_last, dvdt, prime, td, 1, workspace,
                   workspace_floats, (hipStream_t)stream, f.c, &widest);
  if (rc != RIAB_OK) return rc;
  f.v = v;
  f.v_last = v_last;
  f.dvdt = dvdt;
  f.td = td;
  f.mask = mask;
  f.zero_v = zero_v;
  f.B = p->B;
  f.Bp = p->Bp;
  hipLaunchKernelGGL(td_finish_kernel, dim3((unsigned)(f.n_combine + tb)), dim3(256), 0, (hipStream_t)stream, f);
  return (int)hipGetLastError();
}

extern "C" int riab_td_reset(const RiabTDParams* p, const RiabTDLayer* layers, int32_t n_layers, float* const* rows,
                             int32_t n_rows, const uint8_t* mask, riab_stream_t stream) {
  const int rc = td_check(p, layers, n_layers);
  if (rc != RIAB_OK) return rc;
  if (n_rows < 0 || (n_rows > 0 && !rows)) return RIAB_EINVAL;
  if (n_rows > TD_MAX_ROWS) return RIAB_ETOOBIG;
  TDResetArgs a = {};
  int k = 0, tallest = 0;
  for (int l = 0; l < n_layers; ++l, ++k) {
    a.rows[k] = layers[l].trace;
    a.n_rows[k] = layers[l].n_in;
  }
  for (int r = 0; r < n_rows; ++r, ++k) {
    if (!rows[r]) return RIAB_EINVAL;
    if (((uintptr_t)rows[r] & 15)) return RIAB_EALIGN;
    a.rows[k] = rows[r];
    a.n_rows[k] = p->n;
  }
  for (int i = 0; i < k; ++i) tallest = a.n_rows[i] > tallest ? a.n_rows[i] : tallest;
  a.mask = mask;
  a.B = p->B;
  a.Bp = p->Bp;
  const int64_t quads = (int64_t)tallest * p->Bp / 4;
  hipLaunchKernelGGL(td_reset_kernel, dim3((unsigned)((quads + 255) / 256), (unsigned)k), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
