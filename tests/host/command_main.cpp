// command_main.cpp -- the arithmetic of solorl_commands (solorl_amd/csrc/command.hpp) compiled by the host compiler, for
// tests/test_command_host.py and tests/test_command_gpu.py (tests/command_util.py writes and reads the text below).
//
// stdin (floats as the hex bit patterns of their 32 bits, doubles as those of their 64):
//   seed gid0 n D T lo[3] hi[3] obs_scale[3] zero_prob min_lin_norm interval_min interval_max
//   then T lines, one call each:  flags mask obs[n][D]
//       flags: n characters, '1' restart, '0' none, or "-" = restart == NULL;  mask: n characters '1' / '0', or "-" = mask == NULL
//       D == 0: the no-observation form (obs_in == obs_out == NULL), no observation words follow
//   -> per call n lines "row[8] cmd_out[3] obs_out[D + 3]": the env's memory row, its cmd_out and its wide observation row after
//      the call.  The memory rows start zeroed and persist; cmd_out and obs_out are filled with 0xAA bytes in front of every call, so
//      a masked row shows the fill.
// Every row's observation buffers are heap blocks of exactly D and D + 3 floats, so AddressSanitizer sees an access past either.
// The kernel calls the same functions (solorl_command.hip).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../solorl_amd/csrc/command.hpp"

static bool read_double(double& d) {
  unsigned long long w;
  if (std::scanf("%llx", &w) != 1) return false;
  std::memcpy(&d, &w, 8);
  return true;
}

int main() {
  unsigned long long seed;
  long long gid0;
  int n, D, T;
  if (std::scanf("%llu %lld %d %d %d", &seed, &gid0, &n, &D, &T) != 5 || n < 1 || D < 0 || D > solo::CHANNEL_MAX_OBS || T < 1) return 3;
  solo::CommandParams p{};
  p.key = {(unsigned)seed, (unsigned)(seed >> 32), gid0};
  for (double* v : {p.lo, p.hi, p.obs_scale})
    for (int k = 0; k < 3; k++)
      if (!read_double(v[k])) return 3;
  int imin, imax;
  if (!read_double(p.zero_prob) || !read_double(p.min_lin_norm) || std::scanf("%d %d", &imin, &imax) != 2 || imin < 1 || imax < imin) return 3;
  p.interval_min = imin;
  p.span = (unsigned)(imax - imin + 1);
  std::vector<solo::CommandRow> mem(n);
  std::memset(mem.data(), 0, sizeof(solo::CommandRow) * n);
  for (int t = 0; t < T; t++) {
    char flags[4096], mask[4096];
    if (std::scanf("%4095s %4095s", flags, mask) != 2) return 3;
    const bool no_restart = std::strcmp(flags, "-") == 0, no_mask = std::strcmp(mask, "-") == 0;
    if ((!no_restart && (int)std::strlen(flags) != n) || (!no_mask && (int)std::strlen(mask) != n)) return 3;
    for (int i = 0; i < n; i++) {
      std::vector<float> in(D), out(D ? D + 3 : 0);
      for (float& f : in) {
        unsigned w;
        if (std::scanf("%x", &w) != 1) return 3;
        std::memcpy(&f, &w, 4);
      }
      if (D) std::memset(out.data(), 0xAA, sizeof(float) * out.size());
      double cmd[3];
      std::memset(cmd, 0xAA, sizeof(cmd));
      if (no_mask || mask[i] == '1')
        solo::command_row(p, gid0 + i, !no_restart && flags[i] == '1', &mem[i], D, D ? in.data() : nullptr, D ? out.data() : nullptr, cmd);
      unsigned rw[8];
      std::memcpy(rw, &mem[i], 32);
      for (int k = 0; k < 8; k++) std::printf("%08x ", rw[k]);
      for (int k = 0; k < 3; k++) { unsigned long long w; std::memcpy(&w, cmd + k, 8); std::printf("%016llx ", w); }
      for (size_t k = 0; k < out.size(); k++) { unsigned w; std::memcpy(&w, &out[k], 4); std::printf("%08x ", w); }
      std::printf("\n");
    }
  }
  return 0;
}
