// perturb_main.cpp -- the draws of solorl_perturb (solorl_amd/csrc/perturb.hpp) compiled by the host compiler, for tests/test_perturb_host.py.
//
// stdin: one case per line,  seed gid interval_min interval_max a0 .. a5   (seed, gid decimal 64-bit; the six amplitudes as the hex bit
// patterns of doubles: lin x y z, ang x y z).  stdout: one line per case,
//   first_countdown  then for kicks j = 0..3:  six hex bit patterns of the kick's doubles and the countdown to kick j + 1.
// The kernel calls the same functions per env (perturb_kernel, solorl_hip.hip).
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../solorl_amd/csrc/perturb.hpp"

int main() {
  unsigned long long seed, a[6];
  long long gid;
  int imin, imax;
  int cases = 0;
  while (std::scanf("%llu %lld %d %d %llx %llx %llx %llx %llx %llx", &seed, &gid, &imin, &imax, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) == 10) {
    solo::PerturbParams p{};
    p.seed_lo = (unsigned)seed; p.seed_hi = (unsigned)(seed >> 32);
    p.id0 = 0;
    p.interval_min = imin; p.span = (unsigned)imax - (unsigned)imin + 1u;
    for (int k = 0; k < 6; k++) std::memcpy(&p.max_vel[k], &a[k], 8);
    std::printf("%d", solo::perturb_first_countdown(p, gid));
    for (unsigned j = 0; j < 4; j++) {
      double kick[6];
      const int next = solo::perturb_kick(p, gid, j, kick);
      for (int k = 0; k < 6; k++) { unsigned long long b; std::memcpy(&b, &kick[k], 8); std::printf(" %016llx", b); }
      std::printf(" %d", next);
    }
    std::printf("\n");
    cases++;
  }
  return cases > 0 ? 0 : 2;
}
