// termination.hpp -- the row arithmetic of solorl_terminate (include/solorl.h, "Early termination", which holds the table): which of
// the four rules fire on ONE solorl_env_state row, and what a fired row writes into the step's done, reward, info and statistics arrays.
//
// Plain functions of integers and doubles, host and device alike, as command.hpp and perturb.hpp: the kernel of solorl_term.hip calls
// them with one lane per row on words staged in LDS, tests/host/terminate_main.cpp compiles this file alone with the host compiler and
// walks whole rows through terminate_row.  Every product and sum below rounds on its own (the header says so and the tests compare
// bits), so contraction into an FMA is switched off for this file's functions.  No index is computed from a row's data.
#ifndef SOLORL_TERMINATION_HPP
#define SOLORL_TERMINATION_HPP

#include <cstddef>
#include <cstdint>

#include "../../include/solorl.h"

#if defined(__HIPCC__)
#define TERM_HD __host__ __device__ inline
#else
#define TERM_HD inline
#endif
#if defined(__clang__)
#define TERM_NO_CONTRACT _Pragma("clang fp contract(off)")
#define TERM_UNROLL _Pragma("unroll")
#else
#define TERM_NO_CONTRACT
#define TERM_UNROLL
#endif

namespace solo {

constexpr int TERM_STATE_WORDS = sizeof(solorl_env_state) / 8;              // 255
#define TERM_SW(member) ((int)(offsetof(solorl_env_state, member) / 8))
static_assert(sizeof(solorl_env_state) == 2040 && offsetof(solorl_env_state, timestep) % 8 == 0 &&
              offsetof(solorl_env_state, need_reset) == offsetof(solorl_env_state, timestep) + 4 && offsetof(solorl_env_state, contact_mask) % 8 == 0,
              "row of include/solorl.h: whole 8-byte words, timestep and contact_mask each the low half of one");

// The part of a state row that is read, as four contiguous segments: pos.z and quat | q | lambda_prev | dr, treadmill_y and the two words
// of int32 members.  treadmill_y is not read; it lies between dr and timestep, staging it keeps the tail one segment and makes the
// staged row 49 words, an odd stride.  term_in_word: staged word -> word of the state row; term_staged_word: the inverse for the
// words that are staged.
constexpr int TERM_SEG0 = 5, TERM_SEG1 = 12, TERM_SEG2 = 24, TERM_SEG3 = 8;
constexpr int TERM_IN_WORDS = TERM_SEG0 + TERM_SEG1 + TERM_SEG2 + TERM_SEG3;  // 49
static_assert(TERM_SW(quat) == TERM_SW(pos) + 3 && TERM_SW(dr) + TERM_SEG3 == TERM_STATE_WORDS && TERM_SW(timestep) == TERM_SW(dr) + 6 &&
              TERM_SW(contact_mask) == TERM_SW(dr) + 7 && TERM_SEG1 == SOLORL_STATE_MAX_DOF && TERM_SEG2 == SOLORL_STATE_MAX_PRIMS, "the four segments");
TERM_HD constexpr int term_in_word(int w) {
  return w < TERM_SEG0 ? TERM_SW(pos) + 2 + w : w < TERM_SEG0 + TERM_SEG1 ? TERM_SW(q) + (w - TERM_SEG0)
         : w < TERM_SEG0 + TERM_SEG1 + TERM_SEG2 ? TERM_SW(lambda_prev) + (w - TERM_SEG0 - TERM_SEG1) : TERM_SW(dr) + (w - TERM_SEG0 - TERM_SEG1 - TERM_SEG2);
}
TERM_HD constexpr int term_staged_word(int sw) {
  return sw >= TERM_SW(dr) ? TERM_SEG0 + TERM_SEG1 + TERM_SEG2 + (sw - TERM_SW(dr)) : sw >= TERM_SW(lambda_prev) ? TERM_SEG0 + TERM_SEG1 + (sw - TERM_SW(lambda_prev))
         : sw >= TERM_SW(q) ? TERM_SEG0 + (sw - TERM_SW(q)) : sw - (TERM_SW(pos) + 2);
}

template <int ROBOT> struct TermRobot {
  static constexpr int NQ = ROBOT ? 12 : 8;               // act_dim
  static constexpr int NPRIMS = ROBOT ? 24 : 20;          // a Solo8 has no shoulder housings (primitives 20..23)
};

// neither NaN nor +-Inf, by comparisons alone (a NaN fails both)
TERM_HD bool term_finite(double x) { return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; }

// the low int32 of the 8-byte word that holds it (timestep, contact_mask)
TERM_HD int32_t term_low_int(double word) {
  int32_t v[2];
  __builtin_memcpy(v, &word, sizeof(v));
  return v[0];
}

// The rule bits that fire on one row.  ld(w): word w of the state row (TERM_SW offsets; only staged words are asked for).
// A member that is not finite fires nothing: each rule tests the value it compares for finiteness first.
template <int ROBOT, typename LD> TERM_HD unsigned term_rules_fired(LD ld, const solorl_termination& P, double sim_dt) {
  TERM_NO_CONTRACT
  constexpr int NQ = TermRobot<ROBOT>::NQ, NPRIMS = TermRobot<ROBOT>::NPRIMS;
  if (term_low_int(ld(TERM_SW(timestep))) < P.min_steps) return 0u;
  unsigned fired = 0u;
  if (P.rules & SOLORL_TERM_HEIGHT) {
    const double z = ld(TERM_SW(pos) + 2);
    if (term_finite(z) && z < P.min_height) fired |= SOLORL_TERM_HEIGHT;
  }
  if (P.rules & SOLORL_TERM_TILT) {
    const double qx = ld(TERM_SW(quat)), qy = ld(TERM_SW(quat) + 1);
    const double xx = qx * qx, yy = qy * qy;
    const double s = xx + yy;
    const double s2 = 2.0 * s;
    const double up_z = 1.0 - s2;
    if (term_finite(up_z) && up_z < P.min_up_z) fired |= SOLORL_TERM_TILT;
  }
  if (P.rules & SOLORL_TERM_CONTACT) {
    const unsigned bits = P.contact_prims & (unsigned)term_low_int(ld(TERM_SW(contact_mask))) & ((1u << NPRIMS) - 1u);
    bool hit = false;
TERM_UNROLL
    for (int p = 0; p < NPRIMS; p++) {
      if ((bits >> p) & 1u) {
        const double f = ld(TERM_SW(lambda_prev) + p) / sim_dt;
        hit = hit || (term_finite(f) && f >= P.contact_force_min);
      }
    }
    if (hit) fired |= SOLORL_TERM_CONTACT;
  }
  if (P.rules & SOLORL_TERM_JOINT) {
    bool hit = false;
TERM_UNROLL
    for (int j = 0; j < NQ; j++) {
      const double q = ld(TERM_SW(q) + j);
      hit = hit || (term_finite(q) && (q < P.joint_lo[j] || q > P.joint_hi[j]));
    }
    if (hit) fired |= SOLORL_TERM_JOINT;
  }
  return fired;
}

// One LIVE row i of n (a masked row is not the caller's to pass).  done, reward, fired_out: the row's own elements; info (or nullptr)
// and term_stats (or nullptr): the whole arrays, of which column i is touched.
template <int ROBOT, typename LD>
TERM_HD void terminate_row(LD ld, const solorl_termination& P, double sim_dt, size_t n, size_t i, uint8_t* done, float* reward, uint8_t* fired_out,
                           const solorl_info_soa* info, float* term_stats) {
  if (*done != 0) {                                        // the engine ended and reset it: the row holds the new episode
    *fired_out = 0;
    return;
  }
  const unsigned fired = term_rules_fired<ROBOT>(ld, P, sim_dt);
  *fired_out = (uint8_t)fired;
  if (fired == 0u) return;
  const float r = (float)P.terminal_reward;
  *done = 1;
  *reward = r;
  if (info) {
    if (info->timeout) info->timeout[i] = 0;
    if (info->success) info->success[i] = 0;
    if (info->episode_reward) info->episode_reward[i] = r;
    if (info->ep_stats) {                                  // as the engine's own fall rule: one column per env, no atomics
      float* s = info->ep_stats + i;
      s[0] += 1.0f;
      s[n] += r;
      s[2 * n] += (float)term_low_int(ld(TERM_SW(timestep)));
      s[3 * n] += 0.0f;
TERM_UNROLL
      for (int k = 0; k < 5; k++) s[(size_t)(4 + k) * n] += (float)ld(TERM_SW(dr) + k);
    }
  }
  if (term_stats) {
    term_stats[i] += 1.0f;
TERM_UNROLL
    for (int k = 0; k < SOLORL_TERM_RULES; k++)
      if ((fired >> k) & 1u) term_stats[(size_t)(1 + k) * n + i] += 1.0f;
  }
}

// why the entry point refuses *p for this robot and sim_dt, or nullptr.  Host only (the entry point and the host program).
inline const char* term_refusal(const solorl_termination& P, int robot, double sim_dt) {
  const int nq = robot == SOLORL_ROBOT_SOLO12 ? 12 : 8, nprims = robot == SOLORL_ROBOT_SOLO12 ? 24 : 20;
  constexpr unsigned ALL = SOLORL_TERM_HEIGHT | SOLORL_TERM_TILT | SOLORL_TERM_CONTACT | SOLORL_TERM_JOINT;
  if (!(sim_dt > 0.0) || !term_finite(sim_dt)) return "sim_dt must be > 0 and finite";
  if (P.rules == 0u || (P.rules & ~ALL)) return "rules must be a non-empty set of SOLORL_TERM_* bits";
  if (P.min_steps < 0) return "min_steps must be >= 0";
  if ((P.rules & SOLORL_TERM_HEIGHT) && !term_finite(P.min_height)) return "min_height must be finite";
  if ((P.rules & SOLORL_TERM_TILT) && !term_finite(P.min_up_z)) return "min_up_z must be finite";
  if ((P.rules & SOLORL_TERM_CONTACT) && !term_finite(P.contact_force_min)) return "contact_force_min must be finite";
  if (P.contact_force_min < 0.0) return "contact_force_min must be >= 0";
  for (int j = 0; j < nq; j++) {
    if ((P.rules & SOLORL_TERM_JOINT) && (!term_finite(P.joint_lo[j]) || !term_finite(P.joint_hi[j]))) return "joint_lo and joint_hi must be finite";
    if (P.joint_lo[j] > P.joint_hi[j]) return "joint_lo must not exceed joint_hi";
  }
  if ((P.rules & SOLORL_TERM_CONTACT) && (P.contact_prims >> nprims)) return "contact_prims names primitives the robot does not have";
  if (!term_finite(P.terminal_reward)) return "terminal_reward must be finite";
  return nullptr;
}

}  // namespace solo
#endif  // SOLORL_TERMINATION_HPP
