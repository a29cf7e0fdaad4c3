// dyn_main.cpp -- TEST ONLY.  solorl_amd/csrc/dyn_tensors.hpp -- the per-env arithmetic of solorl_dynamics, the same template the HIP
// kernel instantiates -- compiled by g++ for the CPU, as a stand-alone program so that it can also be built with
// -fsanitize=address,undefined and run as a child process (tests/test_dyn_host.py).
//
//   dyn_main IN OUT
// IN:  one solorl_config, an int32 row count n, four bytes of padding, n solorl_env_state rows.
// OUT: n solorl_env_dyn rows.
// Exit status 0 unless a file could not be read or written or the config names no robot.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host_shim.hpp"
#include "../../solorl_amd/csrc/dyn_tensors.hpp"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  solorl_config cfg;
  int32_t head[2];
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(&cfg, sizeof(cfg), 1, f) != 1 || std::fread(head, sizeof(head), 1, f) != 1 || head[0] < 1) {
    std::fprintf(stderr, "cannot read a solorl_config and a row count from %s\n", argv[1]);
    return 2;
  }
  const size_t n = (size_t)head[0];
  std::vector<double> in(n * solo::KIN_STATE_WORDS), out(n * solo::DYN_OUT_WORDS);
  if (std::fread(in.data(), sizeof(double) * solo::KIN_STATE_WORDS, n, f) != n) { std::fprintf(stderr, "%s: fewer than %zu rows\n", argv[1], n); return 2; }
  std::fclose(f);
  if (cfg.robot != SOLORL_ROBOT_SOLO8 && cfg.robot != SOLORL_ROBOT_SOLO12) { std::fprintf(stderr, "robot %d\n", cfg.robot); return 2; }
  for (size_t i = 0; i < n; i++) {
    const double* r = in.data() + i * solo::KIN_STATE_WORDS;
    double* o = out.data() + i * solo::DYN_OUT_WORDS;
    if (cfg.robot == SOLORL_ROBOT_SOLO12) solo::env_dynamics_row<1>(r, o, cfg.use_urdf_inertia != 0, cfg.gravity, cfg.damping);
    else solo::env_dynamics_row<0>(r, o, cfg.use_urdf_inertia != 0, cfg.gravity, cfg.damping);
  }
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double) * solo::DYN_OUT_WORDS, n, f) != n || std::fclose(f) != 0) {
    std::fprintf(stderr, "cannot write %s\n", argv[2]);
    return 2;
  }
  return 0;
}
