// terminate_main.cpp -- the row arithmetic of solorl_terminate (solorl_amd/csrc/termination.hpp) compiled by the host compiler, for
// tests/test_term_host.py and tests/test_term_gpu.py (tests/term_util.py writes and reads the text below).
//
// stdin (floats as the hex bit patterns of their 32 bits, doubles as those of their 64, bytes and ints in decimal):
//   robot n sim_dt check has_mask has_info has_stats
//   rules min_steps contact_prims min_height min_up_z contact_force_min joint_lo[12] joint_hi[12] terminal_reward
//   mask[n] (only with has_mask)
//   done[n] reward[n] fired[n]                            the arrays' contents before the call
//   timeout[n] success[n] episode_reward[n] ep_stats[10][n]   (only with has_info)
//   term_stats[5][n]                                      (only with has_stats)
//   n rows of 255 words
//   check != 0: the entry point's own refusal of the parameters (term_refusal) is asked first; a refused set prints "refused" and ends
// -> the same arrays after the call, in the same order and notation, one array per line.
// As the kernel, the program leaves a masked row alone and walks every other row through terminate_row.  Every array and every state
// row is a heap block of exactly its size, so AddressSanitizer sees an access past any of them.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../solorl_amd/csrc/termination.hpp"

static bool rd64(double& d) {
  unsigned long long w;
  if (std::scanf("%llx", &w) != 1) return false;
  std::memcpy(&d, &w, 8);
  return true;
}
static bool rd32(float& f) {
  unsigned w;
  if (std::scanf("%x", &w) != 1) return false;
  std::memcpy(&f, &w, 4);
  return true;
}
static bool rd8(uint8_t& b) {
  unsigned w;
  if (std::scanf("%u", &w) != 1 || w > 255) return false;
  b = (uint8_t)w;
  return true;
}
static bool rd(std::vector<uint8_t>& v) { for (auto& x : v) if (!rd8(x)) return false; return true; }
static bool rd(std::vector<float>& v) { for (auto& x : v) if (!rd32(x)) return false; return true; }
static void pr(const std::vector<uint8_t>& v) { for (auto x : v) std::printf("%u ", (unsigned)x); std::printf("\n"); }
static void pr(const std::vector<float>& v) {
  for (auto x : v) { unsigned w; std::memcpy(&w, &x, 4); std::printf("%08x ", w); }
  std::printf("\n");
}

int main() {
  int robot, n, check, has_mask, has_info, has_stats;
  double sim_dt;
  if (std::scanf("%d %d", &robot, &n) != 2 || !rd64(sim_dt) || std::scanf("%d %d %d %d", &check, &has_mask, &has_info, &has_stats) != 4 || n < 1 ||
      (robot != 0 && robot != 1))
    return 3;
  solorl_termination P{};
  unsigned rules, prims;
  int min_steps;
  if (std::scanf("%u %d %u", &rules, &min_steps, &prims) != 3) return 3;
  P.rules = rules; P.min_steps = min_steps; P.contact_prims = prims;
  if (!rd64(P.min_height) || !rd64(P.min_up_z) || !rd64(P.contact_force_min)) return 3;
  for (double* v : {P.joint_lo, P.joint_hi})
    for (int j = 0; j < 12; j++)
      if (!rd64(v[j])) return 3;
  if (!rd64(P.terminal_reward)) return 3;
  const size_t N = (size_t)n;
  std::vector<uint8_t> mask(has_mask ? N : 0), done(N), fired(N), timeout(has_info ? N : 0), success(has_info ? N : 0);
  std::vector<float> reward(N), ep_reward(has_info ? N : 0), ep_stats(has_info ? SOLORL_EPSTAT_FIELDS * N : 0), stats(has_stats ? (1 + SOLORL_TERM_RULES) * N : 0);
  if (!rd(mask) || !rd(done) || !rd(reward) || !rd(fired) || !rd(timeout) || !rd(success) || !rd(ep_reward) || !rd(ep_stats) || !rd(stats)) return 3;
  std::vector<std::unique_ptr<double[]>> rows;
  for (size_t i = 0; i < N; i++) {
    rows.emplace_back(new double[solo::TERM_STATE_WORDS]);
    for (int w = 0; w < solo::TERM_STATE_WORDS; w++)
      if (!rd64(rows.back()[w])) return 3;
  }
  if (check && solo::term_refusal(P, robot ? SOLORL_ROBOT_SOLO12 : SOLORL_ROBOT_SOLO8, sim_dt)) {
    std::printf("refused\n");
    return 0;
  }
  solorl_info_soa info{};
  info.timeout = timeout.data(); info.success = success.data(); info.episode_reward = ep_reward.data(); info.ep_stats = ep_stats.data();
  for (size_t i = 0; i < N; i++) {
    if (has_mask && mask[i] == 0) continue;
    const double* row = rows[i].get();
    auto ld = [row](int w) { return row[w]; };
    if (robot) solo::terminate_row<1>(ld, P, sim_dt, N, i, &done[i], &reward[i], &fired[i], has_info ? &info : nullptr, has_stats ? stats.data() : nullptr);
    else solo::terminate_row<0>(ld, P, sim_dt, N, i, &done[i], &reward[i], &fired[i], has_info ? &info : nullptr, has_stats ? stats.data() : nullptr);
  }
  pr(done); pr(reward); pr(fired);
  if (has_info) { pr(timeout); pr(success); pr(ep_reward); pr(ep_stats); }
  if (has_stats) pr(stats);
  return 0;
}
