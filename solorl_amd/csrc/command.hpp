// command.hpp -- the arithmetic of solorl_commands (include/solorl.h, "Velocity commands"): when an env draws a new velocity command,
// the Philox blocks of a draw, and the three observation words of the command it holds.
//
// Plain functions of integers and doubles, host and device alike, as channel.hpp: the kernel of solorl_command.hip calls command_env
// with one lane per env, tests/host/command_main.cpp compiles this file alone with the host compiler and walks whole rows through
// command_row.  Every difference, product and sum below rounds on its own (the header says so and the tests compare bits), so
// contraction into an FMA is switched off for this file's functions.
#ifndef SOLORL_COMMAND_HPP
#define SOLORL_COMMAND_HPP

#include <cstddef>

#include "channel.hpp"

namespace solo {

// last counter word of the commands' stream (the env's own stream uses 1, 2, 3, the kicks 4, the noise 5, the actuator draws 6)
constexpr unsigned COMMAND_STREAM = 7u;
constexpr int COMMAND_INTERVAL_MAX = 1 << 20;

struct CommandParams {
  ChannelKey key;
  double lo[3], hi[3], obs_scale[3];        // vx, vy, yaw rate
  double zero_prob, min_lin_norm;
  int interval_min;
  unsigned span;                            // interval_max - interval_min + 1
};

struct CommandRow {                         // solorl_env_command
  double cmd[3];
  int countdown;
  unsigned draws;
};

// u = (word >> 8) 2^-24: exact
PERTURB_HD double command_uniform(unsigned word) { return (double)(word >> 8) * (1.0 / 16777216.0); }

// draw d = m.draws of env gid: blocks 2d (interval, three components) and 2d + 1 (the zero command)
PERTURB_HD void command_draw(const CommandParams& p, long long gid, CommandRow& m) {
  CHANNEL_NO_CONTRACT
  const unsigned d = m.draws;
  unsigned a[4], b[4];
  channel_block(p.key, gid, 2u * d, COMMAND_STREAM, a);
  channel_block(p.key, gid, 2u * d + 1u, COMMAND_STREAM, b);
  double c[3];
  for (int k = 0; k < 3; k++) {
    const double width = p.hi[k] - p.lo[k];
    const double part = command_uniform(a[1 + k]) * width;
    c[k] = p.lo[k] + part;
  }
  if (command_uniform(b[0]) < p.zero_prob) c[0] = c[1] = c[2] = 0.0;
  const double xx = c[0] * c[0], yy = c[1] * c[1], floor2 = p.min_lin_norm * p.min_lin_norm;
  const double norm2 = xx + yy;
  if (norm2 < floor2) c[0] = c[1] = 0.0;
  for (int k = 0; k < 3; k++) m.cmd[k] = c[k];
  m.draws = d + 1u;
  m.countdown = p.interval_min + (int)(a[0] % p.span);
}

// the draw decision of one call, and the draw if it is due.  (The countdown goes down in unsigned arithmetic: a row whose words were
// written by something else wraps instead of overflowing.)
PERTURB_HD void command_advance(const CommandParams& p, long long gid, bool restart, CommandRow& m) {
  bool draw = restart || m.draws == 0u;
  if (!draw) {
    m.countdown = (int)((unsigned)m.countdown - 1u);
    draw = m.countdown == 0;
  }
  if (draw) command_draw(p, gid, m);
}

// observation word k of the command a row holds: float(cmd_k * obs_scale_k), the product rounded in double first
PERTURB_HD float command_obs_word(const CommandParams& p, const CommandRow& m, int k) {
  CHANNEL_NO_CONTRACT
  const double y = m.cmd[k] * p.obs_scale[k];
  return (float)y;
}

// one live env but for the copy of its D observation words: mem in/out, tail = the row's three command words or nullptr, cmd_out = the
// row's three doubles or nullptr
PERTURB_HD void command_env(const CommandParams& p, long long gid, bool restart, CommandRow* mem, float* tail, double* cmd_out) {
  CommandRow m = *mem;
  command_advance(p, gid, restart, m);
  *mem = m;
  for (int k = 0; k < 3; k++) {
    if (cmd_out) cmd_out[k] = m.cmd[k];
    if (tail) tail[k] = command_obs_word(p, m, k);
  }
}

// one live row as plain memory (the host program): obs_in [D] -> obs_out [D + 3], both or neither
PERTURB_HD void command_row(const CommandParams& p, long long gid, bool restart, CommandRow* mem, int D, const float* obs_in, float* obs_out,
                            double* cmd_out) {
  command_env(p, gid, restart, mem, obs_out ? obs_out + D : nullptr, cmd_out);
  if (obs_out) __builtin_memcpy(obs_out, obs_in, sizeof(float) * (size_t)D);
}

}  // namespace solo
#endif  // SOLORL_COMMAND_HPP
