// What a riab_mlp_forward call DECIDES before it launches (riab_mlp.hip issues it; DESIGN.md's MLP section names this file as
// the one statement of the host's choice): the error it returns, the kernel instantiation, the block, the grid, the LDS
// size, the width of the weight reads per layer and per input population — and, restated from the kernel, which form of
// the layer-0 loop every pass takes and which register-operand tile every later layer runs.  HIP-free text: the library
// compiles it, and tests/native/mlp_logic_host.cpp builds it for the host with g++ (tests/test_mlp_logic_cpu.py, which also
// checks that the cases of tests/mlp_path_cases.py reach every combination below).
// Every input is a plain value in MLPFacts, every outcome a field of MLPDecision; the functions are pure.
#ifndef RIAB_MLP_LOGIC_H
#define RIAB_MLP_LOGIC_H

#include <cstddef>
#include <cstdint>

#include "riab_hip.h"

namespace riab {

constexpr int MLP_MAX_INPUTS = 8;
constexpr int MLP_KT = 16;                                // k of a slab (riab_mfma_slab.h KT; riab_mlp.hip asserts the two agree)
constexpr int MLP_A_FLOATS = 2 * (MLP_KT / 4) * 128 * 4;  // LDS: W slab [buf][rg][row][s], 16 KB; behind it the rates slab
constexpr int64_t MLP_MAX_T = 65535;                      // time rows are the grid's z axis

struct MLPInputFacts {
  int32_t n;       // cells
  bool null;       // inputs[l] == NULL
  unsigned mod16;  // address of inputs[l] mod 16
};

struct MLPLayerFacts {
  int32_t n_in, n_out;
  int32_t act;       // RIAB_ACT_*
  bool null;         // w == NULL
  bool has_bias;
  unsigned w_mod16;  // address of w mod 16
};

struct MLPFacts {
  int32_t n_inputs, n_layers;  // as the caller gave them: entries past MLP_MAX_INPUTS / RIAB_MLP_MAX_LAYERS are never read
  MLPInputFacts in[MLP_MAX_INPUTS];
  MLPLayerFacts layer[RIAB_MLP_MAX_LAYERS];
  int64_t T, B;
  bool out_null;
  unsigned out_mod16;
  int cus;  // compute units of the device
};

struct MLPDecision {
  int rc;  // RIAB_OK, or the error of the first check that fails (nothing below is meaningful then)
  int maxt;  // mlp_kernel<maxt>: the 32-row tiles of the widest activation carried in registers
  int nw;    // waves of a block: 4 or 1
  unsigned grid_x, grid_z;  // blocks of 32 nw positions; time rows
  size_t lds_bytes;
  int vec[RIAB_MLP_MAX_LAYERS];  // 16-byte reads of the layer's w
  int koff[MLP_MAX_INPUTS];      // first column of layer 0's w that input l multiplies
  int vec0[MLP_MAX_INPUTS];      // 16-byte reads of layer 0's w at this input's columns
  // layer 0: passes of 128 rows (more than one only when it is the only layer), and the MT of mlp_first_layer<MT, maxt> in
  // every pass but the last / in the last (the same when there is one)
  int n_pass, mt_full, mt_last;
  // layers >= 1 (entries 1 .. n_layers - 1): mlp_reg_tile<mti, vec> per 32-row output tile
  int mti[RIAB_MLP_MAX_LAYERS], tiles[RIAB_MLP_MAX_LAYERS];
};

// The two small rules the KERNEL applies on the device, restated for the record (riab_mlp.hip, mlp_kernel: the branch on
// `left` in front of mlp_first_layer and `mti` in front of mlp_reg_tile; a comment there names this place).
// MT of a layer-0 pass that has `left` rows to go, in mlp_kernel<maxt>:
inline int mlp_pass_mt(int maxt, int left) {
  if (maxt == 4) return left > 64 ? 4 : (left > 32 ? 2 : 1);
  if (maxt == 2) return left > 32 ? 2 : 1;
  return 1;
}
// 32-row tiles of the activation a layer >= 1 reads:
inline int mlp_mti(int n_in) { return (n_in + 31) >> 5; }

// ---- validation, in the order riab_mlp_forward has always applied it ------------------------------------------------------
inline int mlp_validate(const MLPFacts& f) {
  if (f.out_null || f.n_inputs <= 0 || f.n_layers <= 0 || f.T <= 0 || f.B <= 0) return RIAB_EINVAL;
  if (f.n_inputs > MLP_MAX_INPUTS || f.n_layers > RIAB_MLP_MAX_LAYERS || f.T > MLP_MAX_T) return RIAB_ETOOBIG;
  int64_t k_sum = 0;
  for (int l = 0; l < f.n_inputs; ++l) {
    if (f.in[l].null || f.in[l].n <= 0) return RIAB_EINVAL;
    k_sum += f.in[l].n;
  }
  for (int i = 0; i < f.n_layers; ++i) {
    const MLPLayerFacts& q = f.layer[i];
    if (q.null || q.n_in <= 0 || q.n_out <= 0) return RIAB_EINVAL;
    if (q.act < RIAB_ACT_LINEAR || q.act > RIAB_ACT_SOFTMAX) return RIAB_EINVAL;
    if (i > 0 && q.n_in != f.layer[i - 1].n_out) return RIAB_EINVAL;
  }
  if (k_sum != (int64_t)f.layer[0].n_in) return RIAB_EINVAL;
  for (int i = 0; i + 1 < f.n_layers; ++i)
    if (f.layer[i].n_out > RIAB_MLP_MAX_HIDDEN) return RIAB_ETOOBIG;
  if (f.B % 4 != 0 || f.out_mod16) return RIAB_EALIGN;
  for (int l = 0; l < f.n_inputs; ++l)
    if (f.in[l].mod16) return RIAB_EALIGN;
  return RIAB_OK;
}

// ---- the launch -----------------------------------------------------------------------------------------------------------
inline MLPDecision mlp_decide(const MLPFacts& f) {
  MLPDecision d = {};
  d.rc = mlp_validate(f);
  if (d.rc != RIAB_OK) return d;
  // a row of w starts on a 16-byte boundary only when the base does and n_in % 4 == 0: 16-byte reads then, 4-byte otherwise
  for (int i = 0; i < f.n_layers; ++i) d.vec[i] = (f.layer[i].w_mod16 == 0 && f.layer[i].n_in % 4 == 0) ? 1 : 0;
  // (mlp_w4<true> also needs the first column of a read to be a multiple of 4: an input's columns start at koff)
  int k_sum = 0;
  for (int l = 0; l < f.n_inputs; ++l) {
    d.koff[l] = k_sum;
    d.vec0[l] = (d.vec[0] && k_sum % 4 == 0) ? 1 : 0;
    k_sum += f.in[l].n;
  }
  // Workgroups of four waves (128 positions) when that grid already covers the chip; one wave (32 positions) otherwise, so
  // that a one-row launch at 4096 agents is 128 workgroups, not 32.
  const int64_t wide = (f.B + 127) / 128 * f.T;
  d.nw = wide >= f.cus ? 4 : 1;
  d.grid_x = (unsigned)((f.B + d.nw * 32 - 1) / (d.nw * 32));
  d.grid_z = (unsigned)f.T;
  d.lds_bytes = (size_t)(MLP_A_FLOATS + 2 * (MLP_KT / 4) * (d.nw * 32) * 4) * sizeof(float);
  // the widest activation carried in registers: every hidden width, or the only layer's rows of one pass
  const int32_t out0 = f.layer[0].n_out;
  int widest = f.n_layers == 1 ? (out0 < 128 ? out0 : 128) : 0;
  for (int i = 0; i + 1 < f.n_layers; ++i) widest = f.layer[i].n_out > widest ? f.layer[i].n_out : widest;
  d.maxt = widest > 64 ? 4 : (widest > 32 ? 2 : 1);
  // what the kernel then does with it (mlp_pass_mt, mlp_mti)
  d.n_pass = f.n_layers == 1 ? (out0 + 127) >> 7 : 1;
  d.mt_last = mlp_pass_mt(d.maxt, out0 - ((d.n_pass - 1) << 7));
  d.mt_full = d.n_pass > 1 ? mlp_pass_mt(d.maxt, 128) : d.mt_last;
  for (int i = 1; i < f.n_layers; ++i) {
    d.mti[i] = mlp_mti(f.layer[i].n_in);
    d.tiles[i] = (f.layer[i].n_out + 31) >> 5;
  }
  return d;
}

}  // namespace riab
#endif
