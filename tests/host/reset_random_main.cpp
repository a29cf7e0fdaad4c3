// reset_random_main.cpp -- TEST ONLY.  The row arithmetic of solorl_randomize_reset (solorl_amd/csrc/reset_random.hpp, the same
// templates the HIP kernel instantiates) compiled by the host compiler, for tests/test_reset_host.py and tests/test_reset_gpu.py
// (tests/reset_util.py writes and reads the text below).
//
// stdin (doubles as the hex bit patterns of their 64 bits, bytes and ints in decimal):
//   robot n joint_limit check has_mask
//   seed env_id_offset place_on_ground
//   joint_pos[12] joint_vel[12] lin_vel[3] ang_vel[3] yaw roll pitch clearance
//   mask[n] (only with has_mask)
//   count[n]
//   n rows of 255 words
//   check != 0: the entry point's own refusal of the parameters (reset_refusal) is asked first; a refused set prints "refused" and ends
// -> count[n] on one line, then the n rows, in the same notation.
// As the kernel, the program leaves a masked row and its count alone and walks every other row through reset_row.  Every array and every
// state row is a heap block of exactly its size, so AddressSanitizer sees an access past any of them.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "host_shim.hpp"
#include "../../solorl_amd/csrc/reset_random.hpp"

static bool rd64(double& d) {
  unsigned long long w;
  if (std::scanf("%llx", &w) != 1) return false;
  std::memcpy(&d, &w, 8);
  return true;
}

int main() {
  int robot, n, check, has_mask, place;
  double joint_limit;
  if (std::scanf("%d %d", &robot, &n) != 2 || !rd64(joint_limit) || std::scanf("%d %d", &check, &has_mask) != 2 || n < 1 || (robot != 0 && robot != 1)) return 3;
  solorl_reset_randomization P{};
  unsigned long long seed;
  long long id0;
  if (std::scanf("%llu %lld %d", &seed, &id0, &place) != 3) return 3;
  P.seed = seed; P.env_id_offset = id0; P.place_on_ground = place;
  for (int j = 0; j < 12; j++) if (!rd64(P.joint_pos[j])) return 3;
  for (int j = 0; j < 12; j++) if (!rd64(P.joint_vel[j])) return 3;
  for (int k = 0; k < 3; k++) if (!rd64(P.lin_vel[k])) return 3;
  for (int k = 0; k < 3; k++) if (!rd64(P.ang_vel[k])) return 3;
  if (!rd64(P.yaw) || !rd64(P.roll) || !rd64(P.pitch) || !rd64(P.clearance)) return 3;
  const size_t N = (size_t)n;
  std::unique_ptr<uint8_t[]> mask(new uint8_t[has_mask ? N : 1]);
  std::unique_ptr<uint32_t[]> count(new uint32_t[N]);
  for (size_t i = 0; has_mask && i < N; i++) {
    unsigned b;
    if (std::scanf("%u", &b) != 1 || b > 255) return 3;
    mask[i] = (uint8_t)b;
  }
  for (size_t i = 0; i < N; i++) {
    unsigned long long c;
    if (std::scanf("%llu", &c) != 1 || c > 0xFFFFFFFFull) return 3;
    count[i] = (uint32_t)c;
  }
  std::vector<std::unique_ptr<double[]>> rows;
  for (size_t i = 0; i < N; i++) {
    rows.emplace_back(new double[solo::STATE_WORDS]);
    for (int w = 0; w < solo::STATE_WORDS; w++)
      if (!rd64(rows.back()[w])) return 3;
  }
  if (check && solo::reset_refusal(P, joint_limit)) {
    std::printf("refused\n");
    return 0;
  }
  for (size_t i = 0; i < N; i++) {
    if (has_mask && mask[i] == 0) continue;
    const long long gid = P.env_id_offset + (long long)i;
    if (robot) solo::reset_row<1>(rows[i].get(), &count[i], P, joint_limit, gid);
    else solo::reset_row<0>(rows[i].get(), &count[i], P, joint_limit, gid);
  }
  for (size_t i = 0; i < N; i++) std::printf("%u ", (unsigned)count[i]);
  std::printf("\n");
  for (size_t i = 0; i < N; i++) {
    for (int w = 0; w < solo::STATE_WORDS; w++) {
      unsigned long long b;
      std::memcpy(&b, &rows[i][w], 8);
      std::printf("%016llx ", b);
    }
    std::printf("\n");
  }
  return 0;
}
