// shape_main.cpp -- TEST ONLY.  solorl_amd/csrc/reward_shape.hpp -- the per-env arithmetic of solorl_shape_reward, the same templates
// the HIP kernel instantiates -- compiled by g++ for the CPU, as a stand-alone program so that it can also be built with
// -fsanitize=address,undefined and run as a child process (tests/test_shape_host.py).
//
//   shape_main IN OUT
// IN:  one solorl_config, one solorl_shape_params, an int32 row count n, an int32 flag word (bit 0: a mask follows, bit 1: done flags,
//      bit 2: rewards, bit 3: terms_out, bit 4: ep_out), n solorl_env_state rows, n x act_dim float actions (8 or 12 per row),
//      n solorl_env_shape rows, n float rewards, n x 16 doubles terms_out, 17 x n doubles ep_out, n mask bytes, n done bytes
//      (every array is present whatever the flags say: an absent one is passed as a null pointer and comes back as it was).
// OUT: the n memory rows, n rewards, n x 16 terms_out, 17 x n ep_out, as the call leaves them.
// Exit status 0 unless a file could not be read or written or the config names no robot.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_shim.hpp"
#include "../../solorl_amd/csrc/reward_shape.hpp"

template <typename T> static bool rd(FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T> static bool wr(FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  solorl_config cfg;
  solorl_shape_params P;
  int32_t head[2];
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(&cfg, sizeof(cfg), 1, f) != 1 || std::fread(&P, sizeof(P), 1, f) != 1 || std::fread(head, sizeof(head), 1, f) != 1 || head[0] < 1) {
    std::fprintf(stderr, "cannot read a solorl_config, a solorl_shape_params and a row count from %s\n", argv[1]);
    return 2;
  }
  if (cfg.robot != SOLORL_ROBOT_SOLO8 && cfg.robot != SOLORL_ROBOT_SOLO12) { std::fprintf(stderr, "robot %d\n", cfg.robot); return 2; }
  const bool solo12 = cfg.robot == SOLORL_ROBOT_SOLO12;
  const int act_dim = solo12 ? 12 : 8;
  const size_t n = (size_t)head[0];
  const int flags = head[1];
  std::vector<double> in(n * solo::STATE_WORDS), mem(n * solo::SHAPE_MEM_WORDS), terms(n * solo::SHAPE_TERMS), ep(solo::SHAPE_EP_FIELDS * n);
  std::vector<float> act(n * act_dim), rew(n);
  std::vector<uint8_t> mask(n), done(n);
  if (!rd(f, in) || !rd(f, act) || !rd(f, mem) || !rd(f, rew) || !rd(f, terms) || !rd(f, ep) || !rd(f, mask) || !rd(f, done)) {
    std::fprintf(stderr, "%s: fewer than %zu rows\n", argv[1], n);
    return 2;
  }
  std::fclose(f);
  const double dtc = cfg.sim_dt * (double)cfg.frame_skip;
  for (size_t i = 0; i < n; i++) {
    if ((flags & 1) && !mask[i]) continue;
    const double* r = in.data() + i * solo::STATE_WORDS;
    double* m = mem.data() + i * solo::SHAPE_MEM_WORDS;
    const float* a = act.data() + i * act_dim;               // rows of act_dim floats, as the entry point takes them
    const bool d = (flags & 2) && done[i];
    float* rw = (flags & 4) ? rew.data() + i : nullptr;
    double* t = (flags & 8) ? terms.data() + i * solo::SHAPE_TERMS : nullptr;
    double* e = (flags & 16) ? ep.data() : nullptr;
    if (solo12) solo::env_shape_row<1>(r, m, a, d, rw, t, e, n, i, P, cfg.sim_dt, dtc);
    else solo::env_shape_row<0>(r, m, a, d, rw, t, e, n, i, P, cfg.sim_dt, dtc);
  }
  f = std::fopen(argv[2], "wb");
  if (!f || !wr(f, mem) || !wr(f, rew) || !wr(f, terms) || !wr(f, ep) || std::fclose(f) != 0) {
    std::fprintf(stderr, "cannot write %s\n", argv[2]);
    return 2;
  }
  return 0;
}
