// rows_main.cpp -- TEST ONLY.  solorl_amd/csrc/kinematics.hpp and dyn_tensors.hpp -- the per-env arithmetic of solorl_kinematics and
// solorl_dynamics, the same templates the HIP kernels instantiate -- compiled by g++ for the CPU, as a stand-alone program so that it
// can also be built with -fsanitize=address,undefined and run as a child process (tests/test_kin_host.py, tests/test_dyn_host.py).
//
//   rows_main kin|dyn IN OUT
// IN:  one solorl_config, an int32 row count n, four bytes of padding, n solorl_env_state rows.
// OUT: n solorl_env_kin (kin) or solorl_env_dyn (dyn) rows.
// Exit status 0 unless the query is neither, a file could not be read or written or the config names no robot.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_shim.hpp"
#include "../../solorl_amd/csrc/kinematics.hpp"
#include "../../solorl_amd/csrc/dyn_tensors.hpp"

int main(int argc, char** argv) {
  const bool kin = argc == 4 && !std::strcmp(argv[1], "kin");
  if (!kin && !(argc == 4 && !std::strcmp(argv[1], "dyn"))) { std::fprintf(stderr, "usage: %s kin|dyn IN OUT\n", argv[0]); return 2; }
  solorl_config cfg;
  int32_t head[2];
  FILE* f = std::fopen(argv[2], "rb");
  if (!f || std::fread(&cfg, sizeof(cfg), 1, f) != 1 || std::fread(head, sizeof(head), 1, f) != 1 || head[0] < 1) {
    std::fprintf(stderr, "cannot read a solorl_config and a row count from %s\n", argv[2]);
    return 2;
  }
  const size_t n = (size_t)head[0], out_words = kin ? solo::KIN_OUT_WORDS : solo::DYN_OUT_WORDS;
  std::vector<double> in(n * solo::STATE_WORDS), out(n * out_words);
  if (std::fread(in.data(), sizeof(double) * solo::STATE_WORDS, n, f) != n) { std::fprintf(stderr, "%s: fewer than %zu rows\n", argv[2], n); return 2; }
  std::fclose(f);
  if (cfg.robot != SOLORL_ROBOT_SOLO8 && cfg.robot != SOLORL_ROBOT_SOLO12) { std::fprintf(stderr, "robot %d\n", cfg.robot); return 2; }
  const bool solo12 = cfg.robot == SOLORL_ROBOT_SOLO12, urdf = cfg.use_urdf_inertia != 0;
  for (size_t i = 0; i < n; i++) {
    const double* r = in.data() + i * solo::STATE_WORDS;
    double* o = out.data() + i * out_words;
    if (kin && solo12) solo::env_kinematics_row<1>(r, o, urdf, cfg.sim_dt, cfg.gravity);
    else if (kin) solo::env_kinematics_row<0>(r, o, urdf, cfg.sim_dt, cfg.gravity);
    else if (solo12) solo::env_dynamics_row<1>(r, o, urdf, cfg.gravity, cfg.damping);
    else solo::env_dynamics_row<0>(r, o, urdf, cfg.gravity, cfg.damping);
  }
  f = std::fopen(argv[3], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double) * out_words, n, f) != n || std::fclose(f) != 0) {
    std::fprintf(stderr, "cannot write %s\n", argv[3]);
    return 2;
  }
  return 0;
}
