// critic_obs.hpp -- the privileged words of ONE env's critic row (include/solorl.h solorl_critic_obs, which holds the word table):
// twenty words of the simulator's truth behind the clean observation row, fp64 rounded to float once.
//
// Two pieces, as reward_shape.hpp, whose foot path this file reuses: the four feet's words come from a KinRow (kinematics.hpp) with
// shape_foot_store -- the foot point, its velocity and its force are KinRow's own, not restated -- and critic_priv turns them, the
// row's contact_mask and timestep and the env's command, actuator and kick rows into the twenty words.  solorl_critic.hip runs the
// legs on four wavefronts and critic_priv on the first, one lane per env each; tests/host/critic_main.cpp, compiled by g++ under
// SOLO_HOST_SHIM, calls env_critic_row, which runs them one after the other.  The header promises that the products of words 8..11
// and 19 and of every scale round on their own and the tests compare bits, so contraction into an FMA is switched off in critic_priv.
#pragma once
#include <cstddef>
#include <cstdint>

#include "reward_shape.hpp"

#if defined(__clang__)
#define CRITIC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CRITIC_NO_CONTRACT
#endif

namespace solo {

constexpr int CRITIC_PRIV = SOLORL_CRITIC_PRIV;
constexpr int CRITIC_MAX_OBS = 210;                               // 42 words x (1 + 4 history levels)
static_assert(CRITIC_PRIV == 20 && sizeof(solorl_critic_params) == 8 * CRITIC_PRIV + 8, "the word table and its params of include/solorl.h");
static_assert(offsetof(solorl_env_state, timestep) % 8 == 0 && sizeof(solorl_env_actuator) == 256 && sizeof(solorl_env_command) == 32, "row layouts");

// the part of a state row that is read: what the shaped terms stage (pos .. tau, lambda_prev of the four foot primitives, the
// contact_mask word) and the 8-byte word that holds timestep.  critic_in_word: staged word -> word of the state row; a reader of the
// staged row uses shape_staged_word for the first SHAPE_IN_WORDS and CRITIC_IN_TIME for the last
constexpr int CRITIC_IN_TIME = SHAPE_IN_WORDS;                    // 54
constexpr int CRITIC_IN_WORDS = SHAPE_IN_WORDS + 1;               // 55
SD constexpr int critic_in_word(int w) { return w < SHAPE_IN_WORDS ? shape_in_word(w) : STATE_SW(timestep); }

struct CriticScale { double s[CRITIC_PRIV]; };                    // solorl_critic_params' scale, by value to the kernel

// The twenty words of one row.  foot(k): word k of the feet's 28 words (shape_foot_slot);  cmask, timestep: the row's;  cmd: the env's
// command (vx, vy, yaw rate) or nullptr;  act: the env's actuator row or nullptr;  kick: the env's kick row (6 doubles) or nullptr;
// put(k, v): word E + k of the critic row.
template <int ROBOT, typename FT, typename PUT>
SD void critic_priv(FT foot, int cmask, int timestep, const double* cmd, const solorl_env_actuator* act, const double* kick,
                    const CriticScale& S, PUT put) {
  CRITIC_NO_CONTRACT
  constexpr int A = Robot<ROBOT>::NQ;
  double raw[CRITIC_PRIV];
  static_for<4>([&](auto fc) {
    CRITIC_NO_CONTRACT
    constexpr int f = decltype(fc)::value, w0 = SHAPE_FOOT_WORDS * f;
    const double ux = foot(w0 + 3), uy = foot(w0 + 4);
    const double xx = ux * ux, yy = uy * uy;
    raw[f] = foot(w0 + 6);
    raw[4 + f] = foot(w0 + 2);
    raw[8 + f] = sqrt(xx + yy);
  });
  static_for<3>([&](auto kc) { raw[12 + decltype(kc)::value] = cmd ? cmd[decltype(kc)::value] : 0.0; });
  raw[15] = (double)timestep;
  raw[16] = (double)__builtin_popcount((unsigned)(cmask & shape_collision_bits<ROBOT>()));
  double latency = 0.0, gain = 0.0;
  if (act) {
    latency = (double)act->latency;
    double sum = (double)act->gain[0];
    static_for<A - 1>([&](auto jc) { sum += (double)act->gain[1 + decltype(jc)::value]; });
    gain = sum / (double)A - 1.0;
  }
  raw[17] = latency;
  raw[18] = gain;
  double speed = 0.0;
  if (kick) {
    const double xx = kick[0] * kick[0], yy = kick[1] * kick[1];
    speed = sqrt(xx + yy);
  }
  raw[19] = speed;
  static_for<CRITIC_PRIV>([&](auto kc) {
    CRITIC_NO_CONTRACT
    constexpr int k = decltype(kc)::value;
    const double y = raw[k] * S.s[k];
    put(k, (float)y);
  });
}

// one row given as plain memory (the host program): state row, obs_in [E] -> out [E + 20]
template <int ROBOT> SD void env_critic_row(const double* in, const float* obs_in, int E, const double* cmd, const solorl_env_actuator* act,
                                             const double* kick, const CriticScale& S, double sim_dt, float* out) {
  int32_t cmask, timestep;
  __builtin_memcpy(&cmask, in + KIN_IN_MASK_WORD, sizeof(cmask));
  __builtin_memcpy(&timestep, in + STATE_SW(timestep), sizeof(timestep));
  double feet[SHAPE_FEET_WORDS];
  auto ld = [&](int w) { return in[w]; };
  static_for<4>([&](auto lc) { shape_leg<ROBOT, decltype(lc)::value>(ld, cmask, [&](int k, double v) { feet[k] = v; }, sim_dt); });
  __builtin_memcpy(out, obs_in, sizeof(float) * (size_t)E);
  critic_priv<ROBOT>([&](int k) { return feet[k]; }, cmask, timestep, cmd, act, kick, S, [&](int k, float v) { out[E + k] = v; });
}

}  // namespace solo
