// channel.hpp -- the arithmetic of solorl_obs_noise and solorl_actuate (include/solorl.h, "Observation noise and actuation"): Philox
// block -> noise of an observation component, latency and motor gains of an episode, the delayed and scaled action.
//
// Plain functions of integers, floats and doubles, host and device alike, as perturb.hpp: the kernels of solorl_channel.hip call the
// per-component and per-joint ones, tests/host/channel_main.cpp compiles this file alone with the host compiler and walks whole rows
// through channel_noise_row / channel_actuate_row.  Every product and every sum below rounds on its own (the header says so and the
// tests compare bits), so contraction into an FMA is switched off for this file's functions.
#ifndef SOLORL_CHANNEL_HPP
#define SOLORL_CHANNEL_HPP

#include "perturb.hpp"

#if defined(__clang__)
#define CHANNEL_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CHANNEL_NO_CONTRACT
#endif

namespace solo {

// last counter word of the two streams (the env's own stream uses 1, 2, 3, the kicks 4)
constexpr unsigned NOISE_STREAM = 5u, ACTUATE_STREAM = 6u;
constexpr int CHANNEL_DELAY_MAX = 4;        // SOLORL_DELAY_MAX
constexpr int CHANNEL_MAX_OBS = 210;        // 42 words x (1 + 4 history levels)
// solorl_env_actuator as 64 words: buf[4][12], gain[12], latency, fill, episodes, reserved
constexpr int ACT_ROW_WORDS = 64, ACT_OFF_GAIN = 48, ACT_OFF_LATENCY = 60, ACT_OFF_FILL = 61, ACT_OFF_EPISODES = 62;

struct ChannelKey {
  unsigned seed_lo, seed_hi;
  long long id0;                            // env_id_offset: gid = id0 + i
};

struct ActuateParams {
  ChannelKey key;
  int act_dim, delay_min, delay_max;
  double gain_range;
};

PERTURB_HD void channel_block(const ChannelKey& k, long long gid, unsigned block, unsigned stream, unsigned (&out)[4]) {
  perturb_philox(k.seed_lo, k.seed_hi, (unsigned)gid, (unsigned)((unsigned long long)gid >> 32), block, stream, out);
}

// (2u - 1) with u = (word >> 8) 2^-24: exact
PERTURB_HD double channel_symmetric(unsigned word) {
  CHANNEL_NO_CONTRACT
  const double u = (double)(word >> 8) * (1.0 / 16777216.0);
  return 2.0 * u - 1.0;
}

// ---- observation noise
PERTURB_HD int noise_blocks(int D) { return (D + 3) / 4; }

// block b of call `count` of env gid: words w -> components 4 b + w
PERTURB_HD void noise_block(const ChannelKey& k, long long gid, unsigned count, int B, int b, unsigned (&out)[4]) {
  channel_block(k, gid, count * (unsigned)B + (unsigned)b, NOISE_STREAM, out);
}

// float(double(x) + (2u - 1) double(scale)): the product rounds, then the sum, then the result goes to float.  scale == 0: x's bits
PERTURB_HD float noise_component(unsigned word, float scale, float x) {
  CHANNEL_NO_CONTRACT
  if (scale == 0.0f) return x;
  const double e = channel_symmetric(word) * (double)scale;
  const double y = (double)x + e;
  return (float)y;
}

// one live row, in the kernel's order (host programs and documentation; the kernel spreads the blocks over threads)
PERTURB_HD void channel_noise_row(const ChannelKey& k, long long gid, const float* scale, int D, unsigned* count, const float* in, float* out) {
  const int B = noise_blocks(D);
  const unsigned c0 = *count;
  for (int b = 0; b < B; b++) {
    unsigned r[4];
    noise_block(k, gid, c0, B, b, r);
    for (int w = 0; w < 4 && 4 * b + w < D; w++) {
      const int c = 4 * b + w;
      if (scale[c] != 0.0f || out != in) out[c] = noise_component(r[w], scale[c], in[c]);
    }
  }
  *count = c0 + 1u;
}

// ---- actuation
// episode e of env gid: block 4 e word 0 -> the latency
PERTURB_HD int actuate_latency(const ActuateParams& p, long long gid, unsigned e) {
  unsigned r[4];
  channel_block(p.key, gid, 4u * e, ACTUATE_STREAM, r);
  return p.delay_min + (int)(r[0] % (unsigned)(p.delay_max - p.delay_min + 1));
}

// block 4 e + 1 + j / 4 word j % 4 -> joint j's gain: float(1 + (2u - 1) gain_range), product and sum rounded one after the other
PERTURB_HD float actuate_gain(const ActuateParams& p, long long gid, unsigned e, int j) {
  CHANNEL_NO_CONTRACT
  unsigned r[4];
  channel_block(p.key, gid, 4u * e + 1u + (unsigned)(j >> 2), ACTUATE_STREAM, r);
  const double d = channel_symmetric(r[j & 3]) * p.gain_range;
  const double g = 1.0 + d;
  return (float)g;
}

// the level of buf the delayed action comes from, or -1: the action of this call.  (The clamps change nothing for a row this code wrote;
// they keep a row whose header words were written by something else from addressing memory outside itself.)
PERTURB_HD int actuate_level(int latency, int fill) {
  if (latency <= 0 || fill <= 0) return -1;
  const int level = (latency < fill ? latency : fill) - 1;
  return level < CHANNEL_DELAY_MAX ? level : CHANNEL_DELAY_MAX - 1;
}

PERTURB_HD float actuate_scale(const ActuateParams& p, float gain, float d) {
  CHANNEL_NO_CONTRACT
  if (p.gain_range == 0.0) return d;
  const double y = (double)gain * (double)d;
  return (float)y;
}

PERTURB_HD int actuate_fill(int fill, int delay_max) { return fill + 1 < delay_max ? fill + 1 : delay_max; }

// the integer words of a row share the array with its floats
PERTURB_HD int actuate_word(const float* row, int w) { int v; __builtin_memcpy(&v, row + w, sizeof(v)); return v; }
PERTURB_HD void actuate_set_word(float* row, int w, int v) { __builtin_memcpy(row + w, &v, sizeof(v)); }

// one env, in the kernel's order; row: the env's 64 words (floats and int32 words share the array, as the struct lays them out)
PERTURB_HD void channel_actuate_row(const ActuateParams& p, long long gid, bool restart, float* row, const float* in, float* out) {
  const unsigned e = (unsigned)actuate_word(row, ACT_OFF_EPISODES);
  int latency = actuate_word(row, ACT_OFF_LATENCY), fill = actuate_word(row, ACT_OFF_FILL);
  if (restart || e == 0u) {
    latency = actuate_latency(p, gid, e);
    for (int j = 0; j < p.act_dim; j++) row[ACT_OFF_GAIN + j] = actuate_gain(p, gid, e, j);
    fill = 0;
    actuate_set_word(row, ACT_OFF_LATENCY, latency);
    actuate_set_word(row, ACT_OFF_EPISODES, (int)(e + 1u));
  }
  const int level = actuate_level(latency, fill);
  for (int j = 0; j < p.act_dim; j++) {
    const float a = in[j];
    const float d = level < 0 ? a : row[level * 12 + j];
    out[j] = actuate_scale(p, row[ACT_OFF_GAIN + j], d);
    for (int k = p.delay_max - 1; k > 0; k--) row[k * 12 + j] = row[(k - 1) * 12 + j];
    if (p.delay_max > 0) row[j] = a;
  }
  actuate_set_word(row, ACT_OFF_FILL, actuate_fill(fill, p.delay_max));
}

}  // namespace solo
#endif  // SOLORL_CHANNEL_HPP
