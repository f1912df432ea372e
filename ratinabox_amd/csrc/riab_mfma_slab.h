// The streamed fp32 GEMM core of ff_kernel (riab_ff.hip), gp_kernel (riab_gp.hip) and bayes_kernel (riab_bayes.hip);
// mlp_first_layer (riab_mlp.hip), whose operand A is staged differently, takes the types, KT and swizzle().  gfx950 only.
//
//     acc[mt][row][column] += sum_k A[k][32 mt + row] * X[k][column]
//
// A is an operand with unit stride along its columns ([k][m]: W^T, the training matrix, the table of log rates), X the
// input rows of one time row ([k][position]).  A workgroup is 4 waves and owns NB = 128 positions and 32 MT columns of
// A; wave w owns positions [32w, 32w + 32) and all MT 32-row tiles, so one X fragment read from LDS feeds MT MFMAs.  K
// is walked in slabs of KT = 16 through double-buffered LDS on v_mfma_f32_32x32x2_f32: exact fp32, a k-ordered fmaf
// chain, k ascending over the populations and within each of them.  This comment is the one statement of what follows;
// the kernels refer to it.
//
// FRAGMENTS (lane l, kh = l >> 5, j = l & 31).  A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]; C/D: column
// l & 31, row (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).  Frag holds kh, j and the swizzled LDS columns jb (the lane's
// position) and ja[mt] (its column of A in tile mt).
//
// LDS (SlabTiles).  One slab of an operand is [g][kh][column][s] with k = 8g + 2s + kh, stored as [2g + kh][column][s]:
// the four k-steps a lane needs for one column are one 16-byte read, so a group of 4 MT MFMAs is fed by 1 + MT
// ds_read_b128.  A thread fetches rows k0 + krow + 2s (s = 0..3, krow = 8g + kh) x 4 consecutive columns c4..c4+3 by
// 16-byte loads and transposes them in registers on the way in (transpose_stash: [s][column] -> [column][s]).
//
// SWIZZLE.  Column c lives at swizzle(c) = c ^ ((c >> 3) & 7).  The stash writes 16 bytes per lane, lanes 4 columns
// apart: unswizzled, lanes 2 apart would meet on a bank; the XOR with bits 3..5 of the column (constant over a thread's
// quad, so it costs one value, `sw`) spreads the 8 lanes of a store group over all banks.  The fragment reads of
// consecutive columns stay a permutation within each run of 8 columns, hence conflict-free as well.
//
// BOUNDS.  Every fetch reads a clamped address: a row past K reads row K - 1, a column quad outside the problem reads
// quad 0 (B and the padded width of A are multiples of 4: a quad is wholly inside or outside).  A clamped address is
// always inside the operand, so the fetch is branch-free and in bounds; whatever it read there is replaced by 0 by a
// select in the stash (SlabMask and the row test) before it can reach a product.  The same select zeroes the columns
// of a quad at or past SlabMask::ncols whatever they hold (bayes_kernel's padding bins).  Output rows and columns past
// the problem are computed from those zeros and never stored: the guard bands of every caller rest on this.
//
// BARRIERS.  Two per slab pair suffice.  (1) The caller's __syncthreads() in front of a population's first stash: every
// wave has finished reading the buffer `buf` (the previous population's last slab) and the caller's epilogue tables,
// which the caller rewrites between that barrier and the stash.  (2) The barrier behind each stash: the slab is
// visible before its MFMAs.  The stash into buf ^ 1 needs no barrier of its own in front: that buffer was last read
// one iteration ago, and barrier (2) of that iteration lies between those reads and this write.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace riab {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int KT = 16;    // K slab
constexpr int NB = 128;   // positions per workgroup

__device__ __forceinline__ int swizzle(int c) { return c ^ ((c >> 3) & 7); }

// One thread's share of a slab in registers: rows kbase + 2s (s = 0..3) x 4 consecutive columns.
struct Slab {
  v4f v[4];
};

// The clamped fp32 fetch (BOUNDS): rows kbase + 2s of `src`, `ld` floats apart, columns col..col+3.
template <class Col>
__device__ __forceinline__ Slab fetch_f32(const float* src, int64_t ld, Col col, int K, int kbase) {
  Slab f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int k = kbase + 2 * s;
    const int kc = k < K ? k : K - 1;
    f.v[s] = *reinterpret_cast<const v4f*>(src + (int64_t)kc * ld + col);
  }
  return f;
}

// Which of a thread's fetched values are real (BOUNDS): its column quad lies inside the problem, and columns
// c4 .. c4 + ncols - 1 of it are to be kept (ncols >= 4: all of them).
struct SlabMask {
  bool col_ok;
  int ncols;
};

// 4x4 register transpose [s][column] -> [column][s] into one [column][s] row group of a slab starting at `dst`.  Row s
// is k = kfirst + 2s: rows >= K, a quad outside the problem and its columns past ncols become 0.
__device__ __forceinline__ void transpose_stash(float* dst, const Slab& f, int c4, int kfirst, int K, SlabMask m) {
  const int sw = (c4 >> 3) & 7;   // swizzle() of c4 .. c4 + 3 is an XOR with this
  v4f v[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) v[s] = (m.col_ok && kfirst + 2 * s < K) ? f.v[s] : v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *reinterpret_cast<v4f*>(dst + ((c4 + i) ^ sw) * 4) =
        i < m.ncols ? v4f{v[0][i], v[1][i], v[2][i], v[3][i]} : v4f{0.f, 0.f, 0.f, 0.f};
}

// The double-buffered slabs of both operands for MT output tiles (LDS).
template <int MT>
struct SlabTiles {
  float a[2][KT / 4][MT * 32][4];   // operand A, row group [2g + kh]
  float b[2][KT / 4][NB][4];        // the positions
};

// MFMA role of a lane (FRAGMENTS).
template <int MT>
struct Frag {
  int kh, j, jb, ja[MT];
  __device__ __forceinline__ Frag(int lane, int wave) : kh(lane >> 5), j(lane & 31), jb(swizzle(wave * 32 + (lane & 31))) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) ja[mt] = swizzle(mt * 32 + j);
  }
};

// Fetch / stash role of a thread: waves 0-1 take operand A, waves 2-3 the positions; 32 threads x 4 columns cover 128
// columns of row group rg = 2g + kh.  (With MT < 4 the threads of A whose quad lies past 32 MT columns stash nothing.)
template <int MT>
struct SlabRole {
  bool is_b;     // wave-uniform
  int c4, rg, krow;
  float* dst;    // the thread's row group in buffer 0
  int buf_stride;
  __device__ __forceinline__ SlabRole(SlabTiles<MT>& lds, int tid, int wave)
      : is_b(wave >= 2), c4((tid & 31) * 4), rg((tid >> 5) & 3), krow((rg >> 1) * 8 + (rg & 1)),
        dst(is_b ? &lds.b[0][rg][0][0] : &lds.a[0][rg][0][0]),
        buf_stride(is_b ? (KT / 4) * NB * 4 : (KT / 4) * MT * 32 * 4) {}
  // is the thread's quad one of A's 32 MT columns starting at m0, of which `width` exist?
  __device__ __forceinline__ bool a_quad_ok(int m0, int width) const { return c4 < MT * 32 && m0 + c4 < width; }
  __device__ __forceinline__ void stash(const Slab& f, int buf, int K, int k0, SlabMask m) const {
    if (!is_b && c4 >= MT * 32) return;
    transpose_stash(dst + buf * buf_stride, f, c4, k0 + krow, K, m);
  }
};

struct NoHook {
  __device__ __forceinline__ void operator()(float) const {}
};

// The MFMAs of one slab: `a` and `b` point at the slab ([KT/4][a_cols][4] and [KT/4][b_cols][4]).  hook(b) is called
// once per B fragment element, s ascending inside g ascending: this half-wave's k in ascending order.
template <int MT, class Hook>
__device__ __forceinline__ void mfma_slab(v16f (&acc)[MT], const float* a, int a_cols, const float* b, int b_cols,
                                          const Frag<MT>& fr, Hook& hook) {
#pragma unroll
  for (int g = 0; g < KT / 8; ++g) {
    const v4f bq = *reinterpret_cast<const v4f*>(b + ((2 * g + fr.kh) * b_cols + fr.jb) * 4);
    v4f aq[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) aq[mt] = *reinterpret_cast<const v4f*>(a + ((2 * g + fr.kh) * a_cols + fr.ja[mt]) * 4);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      hook(bq[s]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[mt][s], bq[s], acc[mt], 0, 0, 0);
    }
  }
}

// Contracts one input population of width K into acc.  fetch(kbase) returns the thread's Slab of rows kbase + 2s; `m`
// masks it on its way into LDS.  The caller has passed barrier (1) of BARRIERS; `buf` is the buffer to fill first and
// comes back as the one that was read last.
template <int MT, class Fetch, class Hook = NoHook>
__device__ __forceinline__ void contract_population(SlabTiles<MT>& lds, const SlabRole<MT>& role, const Frag<MT>& fr,
                                                    int& buf, int K, SlabMask m, v16f (&acc)[MT], Fetch fetch,
                                                    Hook hook = Hook{}) {
  role.stash(fetch(role.krow), buf, K, 0, m);
  __syncthreads();
  for (int k0 = 0; k0 < K; k0 += KT) {
    const bool more = k0 + KT < K;  // block-uniform
    Slab nxt;
    if (more) nxt = fetch(k0 + KT + role.krow);
    mfma_slab<MT>(acc, &lds.a[buf][0][0][0], MT * 32, &lds.b[buf][0][0][0], NB, fr, hook);
    if (more) {
      role.stash(nxt, buf ^ 1, K, k0 + KT, m);  // (BARRIERS: no barrier in front)
      __syncthreads();
      buf ^= 1;
    }
  }
}

__device__ __forceinline__ void zero_acc(v16f& acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
}

}  // namespace riab
