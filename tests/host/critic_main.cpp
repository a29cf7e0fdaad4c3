// critic_main.cpp -- TEST ONLY.  solorl_amd/csrc/critic_obs.hpp -- the per-env arithmetic of solorl_critic_obs, the same templates the
// HIP kernel instantiates -- compiled by g++ for the CPU, as a stand-alone program so that it can also be built with
// -fsanitize=address,undefined and run as a child process (tests/test_critic_host.py).
//
//   critic_main IN OUT
// IN:  one solorl_config, one solorl_critic_params, an int32 row count n, an int32 flag word (bit 0: a mask follows, bit 1: command
//      rows, bit 2: actuator rows, bit 3: kick rows), n solorl_env_state rows, n x E float observation rows, n solorl_env_command rows,
//      n solorl_env_actuator rows, n x 6 doubles of kicks, n x (E + 20) floats critic_out as it is before the call, n mask bytes
//      (every array is present whatever the flags say: an absent one is passed as a null pointer).
// OUT: the n x (E + 20) floats critic_out, as the call leaves them.
// Exit status 0 unless a file could not be read or written, the config names no robot or E is out of range.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_shim.hpp"
#include "../../solorl_amd/csrc/critic_obs.hpp"

template <typename T> static bool rd(FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T> static bool wr(FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  solorl_config cfg;
  solorl_critic_params P;
  int32_t head[2];
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(&cfg, sizeof(cfg), 1, f) != 1 || std::fread(&P, sizeof(P), 1, f) != 1 || std::fread(head, sizeof(head), 1, f) != 1 || head[0] < 1) {
    std::fprintf(stderr, "cannot read a solorl_config, a solorl_critic_params and a row count from %s\n", argv[1]);
    return 2;
  }
  if (cfg.robot != SOLORL_ROBOT_SOLO8 && cfg.robot != SOLORL_ROBOT_SOLO12) { std::fprintf(stderr, "robot %d\n", cfg.robot); return 2; }
  if (P.obs_dim < 1 || P.obs_dim > solo::CRITIC_MAX_OBS) { std::fprintf(stderr, "obs_dim %d\n", P.obs_dim); return 2; }
  const bool solo12 = cfg.robot == SOLORL_ROBOT_SOLO12;
  const size_t n = (size_t)head[0], E = (size_t)P.obs_dim, O = E + solo::CRITIC_PRIV;
  const int flags = head[1];
  std::vector<double> in(n * solo::STATE_WORDS), kick(n * 6);
  std::vector<float> obs(n * E), out(n * O);
  std::vector<solorl_env_command> cmd(n);
  std::vector<solorl_env_actuator> act(n);
  std::vector<uint8_t> mask(n);
  if (!rd(f, in) || !rd(f, obs) || !rd(f, cmd) || !rd(f, act) || !rd(f, kick) || !rd(f, out) || !rd(f, mask)) {
    std::fprintf(stderr, "%s: fewer than %zu rows\n", argv[1], n);
    return 2;
  }
  std::fclose(f);
  solo::CriticScale S;
  for (int k = 0; k < solo::CRITIC_PRIV; k++) S.s[k] = P.scale[k];
  for (size_t i = 0; i < n; i++) {
    if ((flags & 1) && !mask[i]) continue;
    const double* r = in.data() + i * solo::STATE_WORDS;
    const double* c = (flags & 2) ? cmd[i].cmd : nullptr;
    const solorl_env_actuator* a = (flags & 4) ? &act[i] : nullptr;
    const double* k = (flags & 8) ? kick.data() + i * 6 : nullptr;
    if (solo12) solo::env_critic_row<1>(r, obs.data() + i * E, (int)E, c, a, k, S, cfg.sim_dt, out.data() + i * O);
    else solo::env_critic_row<0>(r, obs.data() + i * E, (int)E, c, a, k, S, cfg.sim_dt, out.data() + i * O);
  }
  f = std::fopen(argv[2], "wb");
  if (!f || !wr(f, out) || std::fclose(f) != 0) {
    std::fprintf(stderr, "cannot write %s\n", argv[2]);
    return 2;
  }
  return 0;
}
