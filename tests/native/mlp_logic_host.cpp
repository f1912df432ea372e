// Host driver around ratinabox_amd/csrc/riab_mlp_logic.h (test infrastructure, built by tests/test_mlp_logic_cpu.py with
// g++): reads one set of facts per line of standard input and prints the decision riab_mlp_forward would take as one line of
// `key=value` words.  Facts: `in=n[:mod16[:null]]` per input population, `layer=n_in:n_out[:bias[:act[:w_mod16[:null]]]]`
// per layer, T, B, cus, out_mod16, out_null; `n_inputs=` / `n_layers=` override the counts (a call may claim more entries
// than it has).  Missing keys: T = 1, B = 4, 256 compute units, everything aligned, nothing null, bias present, linear.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "riab_mlp_logic.h"

static std::string join(const int* v, int from, int to) {
  std::string s;
  for (int i = from; i < to; ++i) s += (i > from ? "," : "") + std::to_string(v[i]);
  return s.empty() ? "-" : s;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty() || line[0] == '#') continue;
    riab::MLPFacts f = {};
    f.T = 1, f.B = 4, f.cus = 256;
    int n_in = 0, n_l = 0, claim_in = -1, claim_l = -1;
    bool has_claim_in = false, has_claim_l = false;
    std::istringstream words(line);
    std::string w;
    while (words >> w) {
      const size_t eq = w.find('=');
      if (eq == std::string::npos) return 2;
      const std::string k = w.substr(0, eq), v = w.substr(eq + 1);
      const long long x = std::strtoll(v.c_str(), nullptr, 0);
      if (k == "in") {
        int n = 0, mod = 0, null = 0;
        if (std::sscanf(v.c_str(), "%d:%d:%d", &n, &mod, &null) < 1) return 2;
        if (n_in < riab::MLP_MAX_INPUTS) f.in[n_in] = riab::MLPInputFacts{n, null != 0, (unsigned)mod};
        ++n_in;
      } else if (k == "layer") {
        int a = 0, b = 0, bias = 1, act = 0, mod = 0, null = 0;
        if (std::sscanf(v.c_str(), "%d:%d:%d:%d:%d:%d", &a, &b, &bias, &act, &mod, &null) < 2) return 2;
        if (n_l < RIAB_MLP_MAX_LAYERS) f.layer[n_l] = riab::MLPLayerFacts{a, b, act, null != 0, bias != 0, (unsigned)mod};
        ++n_l;
      }
      else if (k == "T") f.T = x;
      else if (k == "B") f.B = x;
      else if (k == "cus") f.cus = (int)x;
      else if (k == "out_mod16") f.out_mod16 = (unsigned)x;
      else if (k == "out_null") f.out_null = x != 0;
      else if (k == "n_inputs") claim_in = (int)x, has_claim_in = true;
      else if (k == "n_layers") claim_l = (int)x, has_claim_l = true;
      else return 2;
    }
    f.n_inputs = has_claim_in ? claim_in : n_in;
    f.n_layers = has_claim_l ? claim_l : n_l;
    const riab::MLPDecision d = riab::mlp_decide(f);
    if (d.rc) {
      std::printf("rc=%d\n", d.rc);
      continue;
    }
    // the MT of every layer-0 pass, by the rule the record restates
    std::string passes;
    for (int p = 0; p < d.n_pass; ++p) passes += (p ? "," : "") + std::to_string(p + 1 < d.n_pass ? d.mt_full : d.mt_last);
    std::printf("rc=0 maxt=%d nw=%d grid_x=%u grid_z=%u lds=%zu vec=%s koff=%s vec0=%s passes=%s mti=%s tiles=%s\n", d.maxt, d.nw,
                d.grid_x, d.grid_z, d.lds_bytes, join(d.vec, 0, f.n_layers).c_str(), join(d.koff, 0, f.n_inputs).c_str(),
                join(d.vec0, 0, f.n_inputs).c_str(), passes.c_str(), join(d.mti, 1, f.n_layers).c_str(),
                join(d.tiles, 1, f.n_layers).c_str());
  }
  return 0;
}
