// Host driver around ratinabox_amd/csrc/riab_simulate_logic.h (test infrastructure, built by tests/test_simulate_logic_cpu.py
// with g++): reads one set of facts per line of standard input — `key=value` words, every missing key at the default of a
// new streamer and of the residency cases' call, populations as `pop=kind:n:spikes:stream_supported` — takes the decision in
// the order riab_simulate takes it, and prints it as one line of `key=value` words.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "riab_simulate_logic.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty() || line[0] == '#') continue;
    riab::SimFacts f = {};
    std::vector<riab::SimPop> pops;
    f.T = 16, f.B = 256, f.timed_pop = -1, f.timing_mode = RIAB_TIMING_STAMPS;
    f.strict_opt = 2, f.gate_mode = RIAB_GATE_RESERVED, f.poll_max = 65535, f.head_rows = 256;
    f.same_stream = true, f.n_walls = 4, f.idle = f.reservable = f.side_differs = true;
    bool state_published = true, fail = false;
    std::istringstream words(line);
    std::string w;
    while (words >> w) {
      const size_t eq = w.find('=');
      if (eq == std::string::npos) return 2;
      const std::string k = w.substr(0, eq), v = w.substr(eq + 1);
      const long long x = std::strtoll(v.c_str(), nullptr, 0);
      if (k == "pop") {
        int kind = 0, n = 0, spikes = 0, ok = 0;
        if (std::sscanf(v.c_str(), "%d:%d:%d:%d", &kind, &n, &spikes, &ok) != 4) return 2;
        pops.push_back({kind, n, spikes != 0, ok != 0});
      }
      else if (k == "T") f.T = (int32_t)x;
      else if (k == "B") f.B = x;
      else if (k == "step0") f.step0 = (uint64_t)x;
      else if (k == "forced") f.forced = x != 0;
      else if (k == "capturing") f.capturing = x != 0;
      else if (k == "timed_pop") f.timed_pop = (int32_t)x;
      else if (k == "timing_mode") f.timing_mode = (int32_t)x;
      else if (k == "strict_opt") f.strict_opt = (int)x;
      else if (k == "gate_mode") f.gate_mode = (int)x;
      else if (k == "poll_max") f.poll_max = (int)x;
      else if (k == "head_rows") f.head_rows = (int)x;
      else if (k == "has_side_own") f.has_side_own = x != 0;
      else if (k == "calibrated") f.calibrated = x != 0;
      else if (k == "resync") f.resync = x != 0;
      else if (k == "captured_once") f.captured_once = x != 0;
      else if (k == "step_ns_cfg") f.step_ns_cfg = x;
      else if (k == "step_ns_meas") f.step_ns_meas = x;
      else if (k == "lead_mbps_cfg") f.lead_mbps_cfg = x;
      else if (k == "lead_mbps_meas") f.lead_mbps_meas = x;
      else if (k == "progress_valid") f.progress_valid = x != 0;
      else if (k == "same_ctrl") f.same_ctrl = x != 0;
      else if (k == "same_stream") f.same_stream = x != 0;
      else if (k == "progress_end") f.progress_end = (uint32_t)x;
      else if (k == "pairs") f.pairs = (size_t)x;
      else if (k == "n_walls") f.n_walls = (int32_t)x;
      else if (k == "polygon") f.polygon = (int32_t)x;
      else if (k == "periodic") f.periodic = (int32_t)x;
      else if (k == "hole_mask") f.hole_mask = (uint64_t)x;
      else if (k == "idle") f.idle = x != 0;
      else if (k == "reservable") f.reservable = x != 0;
      else if (k == "side_differs") f.side_differs = x != 0;
      else if (k == "state_published") state_published = x != 0;
      else if (k == "fail") fail = x != 0;
      else return 2;
    }
    f.n_pops = (int32_t)pops.size();
    f.pops = pops.data();
    riab::SimDecision d = {};
    riab::decide_mode(f, d);
    if (d.rc) {
      std::printf("rc=%d strict=%d\n", d.rc, (int)d.strict);
      continue;
    }
    riab::choose_lead(f, d);
    const int candidate = d.lead;
    const bool calibration_due = riab::calibration_due(f, d);
    riab::decide_form(f, d);
    riab::decide_residency(f, d);
    std::string sched;
    for (size_t i = 0; i < d.sched.size(); ++i) sched += (i ? "," : "") + std::to_string(d.sched[i]);
    std::printf("rc=0 strict=%d form=%d candidate=%d calibration_due=%d lead=%d head=%d pure=%d lead_row_bytes=%lld row_ns=%.3f "
                "margin=%.1f step_ns=%.3f sched=%s timing=%d pairs_needed=%zu open=%d resync_next=%d fork=%d monotonic=%d quiet=%d "
                "reserve=%d gate=%d events=%d stamps=%d serial_rows=%u launches=%d join=%d\n",
                (int)d.strict, d.form, candidate, (int)calibration_due, d.lead, d.head, (int)d.pure, (long long)d.lead_row_bytes,
                d.row_ns, d.margin, d.step_ns, sched.empty() ? "-" : sched.c_str(), (int)d.timing, d.pairs_needed, (int)d.open,
                (int)d.resync_next, (int)d.fork, (int)d.monotonic, (int)d.quiet, (int)d.reserve, (int)d.gate, (int)d.events,
                (int)d.stamps, d.serial_rows, riab::planned_launches(f, d), (int)riab::needs_join(d, state_published, fail));
  }
  return 0;
}
