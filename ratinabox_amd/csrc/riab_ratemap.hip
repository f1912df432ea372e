// riab_ratemap.hip — empirical rate maps and the occupancy heatmap from the device-resident history.
//
// Replaces the host route of Neurons.plot_rate_map(method="history") (Neurons.py:377-398, 479-490) and
// Agent.plot_position_heatmap (Agent.py:951-956), both of which go through utils.bin_data_for_histogramming
// (utils.py:544-589) = np.histogram2d with explicit edges.
//
// Two stages, so that the bin of a sample is found once and not once per cell:
//   A  bin_index_kernel   trajectory rows [T][8][Bp] -> one uint16 bin id per (step, agent) + the occupancy counts
//                         (integer atomics: exact and order-free).
//   B  rate_map_kernel    a population's rows [T][n][Bp] (fp32 rates or uint8 spikes) + the bin ids -> per-cell sums.
//                         A wave owns ONE cell and ONE block of time steps and adds into an accumulator of its own in
//                         LDS, in float64 from the first add on (RIAB_RATEMAP_FP32_RUN = 0).  No other wave touches
//                         that accumulator, so no barrier is needed and no floating-point atomic ever goes to memory
//                         that two waves add into.  The wave stores its accumulator as a float64 slab; slab_reduce_kernel
//                         then adds the slabs of a cell in the order of their time blocks into the caller's sums.
//                         The partition into time blocks depends on the shape alone: same inputs, same bits.
//   finish_kernel         sums / max(count, 1) (or the sums) and zero_bins.
//
// Bin ids are stored ORIENTED: id = (ny - 1 - ky) * nx + kx, so sums [n][ny][nx] and counts [ny][nx] already are the
// reference's `heatmap.T[::-1, :]`.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "riab_hip.h"

namespace {

constexpr int kBlock = 256;
constexpr uint16_t kDropped = RIAB_RATEMAP_DROPPED;

// searchsorted(e, x, side="right") - 1 with np.histogram's closed last bin; -1 = outside or NaN.  The guess from the
// mean bin width is corrected against the edges themselves, so the result is the searchsorted one whatever rounding
// np.arange left in them.
__device__ __forceinline__ int bin_of(double x, const double* __restrict__ e, int nb, double inv_width) {
  if (!(x >= e[0]) || !(x <= e[nb])) return -1;
  const double g = (x - e[0]) * inv_width;
  int k = (int)fmin(fmax(g, 0.0), (double)(nb - 1));
  while (k > 0 && x < e[k]) --k;
  while (k < nb - 1 && x >= e[k + 1]) ++k;
  return k;
}

// edges: device [nx + 1] then [ny + 1].  One thread per 4 agents of one step.
__global__ void __launch_bounds__(kBlock) bin_index_kernel(const float* __restrict__ hist, uint32_t quads, uint32_t Q,
                                                           int64_t Bp, int64_t n_real, const double* __restrict__ edges,
                                                           int nx, int ny, uint16_t* __restrict__ ids,
                                                           unsigned long long* __restrict__ counts) {
  extern __shared__ uint32_t h[];
  const int nbins = nx * ny;
  for (int i = threadIdx.x; i < nbins; i += kBlock) h[i] = 0;
  __syncthreads();
  const double* ex = edges;
  const double* ey = edges + nx + 1;
  const double invx = (double)nx / (ex[nx] - ex[0]);
  const double invy = (double)ny / (ey[ny] - ey[0]);
  for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s < quads; s += gridDim.x * kBlock) {
    const uint32_t t = s / Q, q = s - t * Q;
    const float* row = hist + (int64_t)t * RIAB_HIST_ROWS * Bp + (int64_t)q * 4;
    const float4 x4 = *reinterpret_cast<const float4*>(row + RIAB_H_POS_X * Bp);
    const float4 y4 = *reinterpret_cast<const float4*>(row + RIAB_H_POS_Y * Bp);
    const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, ys[4] = {y4.x, y4.y, y4.z, y4.w};
    uint16_t out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      out[j] = kDropped;
      if ((int64_t)q * 4 + j < n_real) {
        const int kx = bin_of((double)xs[j], ex, nx, invx);
        const int ky = bin_of((double)ys[j], ey, ny, invy);
        if (kx >= 0 && ky >= 0) {
          const int id = (ny - 1 - ky) * nx + kx;
          out[j] = (uint16_t)id;
          atomicAdd(&h[id], 1u);
        }
      }
    }
    *reinterpret_cast<ushort4*>(ids + (int64_t)t * Bp + (int64_t)q * 4) = make_ushort4(out[0], out[1], out[2], out[3]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += kBlock)
    if (h[i]) atomicAdd(&counts[i], (unsigned long long)h[i]);
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename T> struct Quad;
template <> struct Quad<float> {
  typedef f32x4 type;
  static __device__ __forceinline__ void widen(const f32x4& v, double* w) { w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
};
template <> struct Quad<uint8_t> {
  typedef uint32_t type;
  static __device__ __forceinline__ void widen(const uint32_t& v, double* w) {
    w[0] = v & 255u; w[1] = (v >> 8) & 255u; w[2] = (v >> 16) & 255u; w[3] = v >> 24;
  }
};

constexpr int kUnroll = 4;

// grid (ceil(n / waves per block), time blocks); dynamic LDS: waves per block * nbins doubles.
template <typename T>
__global__ void __launch_bounds__(kBlock) rate_map_kernel(const T* __restrict__ rows, const uint16_t* __restrict__ ids,
                                                          int64_t Tn, int32_t n, int64_t Bp, uint32_t Q, int64_t Tb,
                                                          int32_t nbins, double* __restrict__ slabs) {
  extern __shared__ double acc_all[];
  typedef typename Quad<T>::type V;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.x * (blockDim.x >> 6) + wave;
  if (c >= n) return;   // (no barrier below: a wave's accumulator is its own)
  double* acc = acc_all + (size_t)wave * nbins;
  for (int i = lane; i < nbins; i += 64) acc[i] = 0.0;
  const int64_t t0 = (int64_t)blockIdx.y * Tb;
  const int64_t t1 = t0 + Tb < Tn ? t0 + Tb : Tn;
  const uint32_t quads = (uint32_t)((t1 - t0) * Q);
  const T* base = rows + (t0 * n + c) * Bp;
  const uint16_t* idb = ids + t0 * Bp;
  const int64_t step = (int64_t)n * Bp;
  for (uint32_t s0 = 0; s0 < quads; s0 += 64 * kUnroll) {
    V v[kUnroll];
    ushort4 b[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint32_t s = s0 + u * 64 + lane;
      if (s < quads) {
        const uint32_t t = s / Q, q = s - t * Q;
        v[u] = __builtin_nontemporal_load(reinterpret_cast<const V*>(base + t * step + (int64_t)q * 4));
        b[u] = *reinterpret_cast<const ushort4*>(idb + (int64_t)t * Bp + (int64_t)q * 4);
      } else {
        b[u] = make_ushort4(kDropped, kDropped, kDropped, kDropped);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      double w[4] = {0.0, 0.0, 0.0, 0.0};
      if (s0 + u * 64 + lane < quads) Quad<T>::widen(v[u], w);
      const uint16_t id[4] = {b[u].x, b[u].y, b[u].z, b[u].w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (id[j] < nbins) atomicAdd(&acc[id[j]], w[j]);   // (an id >= nbins is a dropped sample; nothing is read of it)
    }
  }
  double* out = slabs + ((int64_t)blockIdx.y * n + c) * nbins;
  for (int i = lane; i < nbins; i += 64) out[i] = acc[i];
}

// sums[c][bin] += slab[0][c][bin] + slab[1][c][bin] + ... in that order
__global__ void __launch_bounds__(kBlock) slab_reduce_kernel(const double* __restrict__ slabs, int64_t cells, int32_t n_slabs,
                                                             double* __restrict__ sums) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= cells) return;
  double a = slabs[i];
  for (int k = 1; k < n_slabs; ++k) a += slabs[(int64_t)k * cells + i];
  sums[i] += a;
}

__global__ void __launch_bounds__(kBlock) finish_kernel(const double* __restrict__ sums, const unsigned long long* __restrict__ counts,
                                                        int32_t n, int32_t nbins, int norm, double* __restrict__ maps,
                                                        uint8_t* __restrict__ zero_bins) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < nbins && zero_bins) zero_bins[i] = counts[i] == 0;
  if (i >= (int64_t)n * nbins) return;
  const unsigned long long k = counts[i % nbins];
  maps[i] = norm ? sums[i] / (double)(k ? k : 1ull) : sums[i];
}

// how stage B cuts T steps into time blocks: enough waves to fill the chip, enough samples per wave to pay for clearing
// and storing its accumulator.  A function of the shape alone.
int64_t time_block_rows(int64_t T, int32_t n, int64_t Bp, int32_t nbins) {
  const int64_t Q = Bp / 4;
  int64_t blocks = 4096 / n;
  const int64_t min_quads = nbins > 1024 ? nbins : 1024;
  const int64_t by_work = T * Q / min_quads;
  if (blocks > by_work) blocks = by_work;
  if (blocks > 64) blocks = 64;
  if (blocks < 1) blocks = 1;
  if (blocks > T) blocks = T;
  return (T + blocks - 1) / blocks;
}

int check_edges(const double* e, int32_t nb) {
  if (!e || nb < 1) return RIAB_EINVAL;
  for (int32_t i = 0; i < nb; ++i)
    if (!(e[i] < e[i + 1])) return RIAB_EINVAL;   // (NaN edges fail too)
  return RIAB_OK;
}

int check_grid(int32_t nx, int32_t ny) {
  if (nx < 1 || ny < 1) return RIAB_EINVAL;
  if ((int64_t)nx * ny > RIAB_RATEMAP_MAX_BINS) return RIAB_EUNSUPPORTED;
  return RIAB_OK;
}

}  // namespace

extern "C" int riab_history_bin_index(const float* hist, int64_t T, int64_t B, int64_t n_real, const double* edges_x,
                                      int32_t nx, const double* edges_y, int32_t ny, const double* edges_dev,
                                      uint16_t* bin_ids, int64_t* counts, riab_stream_t stream) {
  if (!hist || !edges_x || !edges_y || !edges_dev || !bin_ids || !counts || T < 0 || B <= 0 || n_real < 0 || n_real > B)
    return RIAB_EINVAL;
  if ((B & 3) || ((uintptr_t)hist & 15) || ((uintptr_t)bin_ids & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)edges_dev & 7))
    return RIAB_EALIGN;
  if (nx < 1 || ny < 1) return RIAB_EINVAL;
  int rc = check_edges(edges_x, nx);
  if (rc == RIAB_OK) rc = check_edges(edges_y, ny);
  if (rc == RIAB_OK) rc = check_grid(nx, ny);
  if (rc != RIAB_OK) return rc;
  const int64_t Q = B / 4, quads = T * Q;
  if (quads >= 0x7fffffffLL) return RIAB_ETOOBIG;
  if (T == 0) return RIAB_OK;
  int64_t blocks = (quads + kBlock - 1) / kBlock;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(bin_index_kernel, dim3((unsigned)blocks), dim3(kBlock), (size_t)nx * ny * sizeof(uint32_t),
                     (hipStream_t)stream, hist, (uint32_t)quads, (uint32_t)Q, B, n_real, edges_dev, nx, ny, bin_ids,
                     reinterpret_cast<unsigned long long*>(counts));
  return (int)hipGetLastError();
}

extern "C" int64_t riab_history_rate_map_workspace(int64_t T, int32_t n, int64_t B, int32_t n_bins) {
  if (T < 0 || n < 1 || B <= 0 || n_bins < 1) return RIAB_EINVAL;
  if (B & 3) return RIAB_EALIGN;
  if (n_bins > RIAB_RATEMAP_MAX_BINS) return RIAB_EUNSUPPORTED;
  if (T * (B / 4) >= 0x7fffffffLL) return RIAB_ETOOBIG;
  if (T == 0) return 0;
  const int64_t Tb = time_block_rows(T, n, B, n_bins);
  return (T + Tb - 1) / Tb * n * n_bins;
}

extern "C" int riab_history_rate_map(const void* rows, int32_t rows_are_spikes, int64_t T, int32_t n, int64_t B,
                                     const uint16_t* bin_ids, int32_t n_bins, double* sums, double* workspace,
                                     int64_t workspace_doubles, riab_stream_t stream) {
  if (!rows || !bin_ids || !sums || !workspace || T < 0 || n < 1 || B <= 0 || n_bins < 1) return RIAB_EINVAL;
  if ((B & 3) || ((uintptr_t)rows & (rows_are_spikes ? 3 : 15)) || ((uintptr_t)bin_ids & 7) || ((uintptr_t)sums & 7) ||
      ((uintptr_t)workspace & 7))
    return RIAB_EALIGN;
  if (n_bins > RIAB_RATEMAP_MAX_BINS) return RIAB_EUNSUPPORTED;
  const int64_t Q = B / 4;
  if (T * Q >= 0x7fffffffLL) return RIAB_ETOOBIG;
  if (T == 0) return RIAB_OK;
  const int64_t Tb = time_block_rows(T, n, B, n_bins);
  const int64_t n_slabs = (T + Tb - 1) / Tb;
  if (workspace_doubles < n_slabs * n * n_bins) return RIAB_EINVAL;
  // 4 waves per workgroup while their float64 accumulators fit 64 KiB of LDS, 2 for the largest grids
  const int waves = n_bins <= 2048 ? 4 : 2;
  const dim3 grid((unsigned)((n + waves - 1) / waves), (unsigned)n_slabs), block(64 * waves);
  const size_t lds = (size_t)waves * n_bins * sizeof(double);
  if (rows_are_spikes)
    hipLaunchKernelGGL(rate_map_kernel<uint8_t>, grid, block, lds, (hipStream_t)stream, (const uint8_t*)rows, bin_ids, T, n,
                       B, (uint32_t)Q, Tb, n_bins, workspace);
  else
    hipLaunchKernelGGL(rate_map_kernel<float>, grid, block, lds, (hipStream_t)stream, (const float*)rows, bin_ids, T, n, B,
                       (uint32_t)Q, Tb, n_bins, workspace);
  int err = (int)hipGetLastError();
  if (err) return err;
  const int64_t cells = (int64_t)n * n_bins;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, workspace, cells, (int32_t)n_slabs, sums);
  return (int)hipGetLastError();
}

extern "C" int riab_history_rate_map_finish(const double* sums, const int64_t* counts, int32_t n, int32_t n_bins,
                                            int32_t norm_by_bincount, double* maps, uint8_t* zero_bins,
                                            riab_stream_t stream) {
  if (!counts || n < 0 || n_bins < 1 || (n > 0 && (!sums || !maps)) || (n == 0 && !zero_bins)) return RIAB_EINVAL;
  if (((uintptr_t)sums & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)maps & 7)) return RIAB_EALIGN;
  if (n_bins > RIAB_RATEMAP_MAX_BINS) return RIAB_EUNSUPPORTED;
  const int64_t cells = (int64_t)(n > 0 ? n : 1) * n_bins;
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     sums, reinterpret_cast<const unsigned long long*>(counts), n, n_bins, norm_by_bincount ? 1 : 0, maps,
                     zero_bins);
  return (int)hipGetLastError();
}
