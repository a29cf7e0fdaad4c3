// reward_shape.hpp -- the shaped reward terms of ONE env (include/solorl.h solorl_shape_reward, which holds the term table): sixteen
// terms of the state row after a step, the step's actions and the env's solorl_env_shape memory row, all in fp64.
//
// Two pieces.  shape_foot_store: the store functor a KinRow (kinematics.hpp) is instantiated with here -- it keeps the seven words of
// a leg's foot primitive (prim_point, prim_vel, prim_force of primitive 13 + 2 leg) and drops every other word of solorl_env_kin, so
// what a leg computes for the dropped words is dead code; the foot point, its velocity and its force are KinRow's own, not restated.
// shape_row: the terms, the reward, the memory row and the episode sums of one row, from R0 (a KinRow's, the same constructor) and
// the four feet's words.  solorl_shape.hip runs the legs on four wavefronts and shape_row on the first, one lane per env each;
// tests/host/shape_main.cpp, compiled by g++ under SOLO_HOST_SHIM, calls env_shape_row, which runs them one after the other.  Every
// row is read and written through ld / st style functors with compile-time word indices: LDS at immediate offsets on the device.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kinematics.hpp"

#ifdef SOLO_HOST_SHIM
using std::exp;
#endif

namespace solo {

constexpr int SHAPE_TERMS = SOLORL_SHAPE_TERMS;
constexpr int SHAPE_MEM_WORDS = sizeof(solorl_env_shape) / 8;     // 45
constexpr int SHAPE_FOOT_WORDS = 7;                               // point x y z, velocity x y z, normal force
constexpr int SHAPE_FEET_WORDS = 4 * SHAPE_FOOT_WORDS;
constexpr int SHAPE_EP_FIELDS = 1 + SHAPE_TERMS;                  // ep_out: the episode count, then the terms' weighted sums
#define SHAPE_MW(member) ((int)(offsetof(solorl_env_shape, member) / 8))
static_assert(sizeof(solorl_env_shape) == 360 && offsetof(solorl_env_shape, prev_contact) % 8 == 0 &&
              offsetof(solorl_env_shape, valid) == offsetof(solorl_env_shape, prev_contact) + 4, "memory row of include/solorl.h: 44 doubles and one word of two int32");
static_assert(SHAPE_TERMS == 16, "the term table");

// the part of a state row that is read: pos .. tau (one contiguous segment), lambda_prev of the four foot primitives, and the 8-byte
// word that holds contact_mask.  shape_in_word: staged word -> word of the state row; shape_staged_word: the inverse, for a reader
// of the staged row (a word that is not staged gives a staged index all the same: its load is dead code, and stays in bounds if kept)
constexpr int SHAPE_IN_HEAD_WORDS = offsetof(solorl_env_state, lambda_prev) / 8;                  // 49
constexpr int SHAPE_IN_WORDS = SHAPE_IN_HEAD_WORDS + 4 + 1;                                       // 54
constexpr int shape_foot_prim(int f) { return 13 + 2 * f; }
SD constexpr int shape_in_word(int w) {
  return w < SHAPE_IN_HEAD_WORDS ? w : w < SHAPE_IN_HEAD_WORDS + 4 ? STATE_SW(lambda_prev) + shape_foot_prim(w - SHAPE_IN_HEAD_WORDS) : KIN_IN_MASK_WORD;
}
SD constexpr int shape_staged_word(int sw) {
  const int p = sw - STATE_SW(lambda_prev);
  return sw < SHAPE_IN_HEAD_WORDS ? sw : (p >= 13 && p <= 19) ? SHAPE_IN_HEAD_WORDS + (p - 13) / 2 : SHAPE_IN_HEAD_WORDS;
}

// word kw of solorl_env_kin -> 7 f + (0..2 point, 3..5 velocity, 6 force) if it belongs to foot f's primitive, else -1
SD constexpr int shape_foot_slot(int kw) {
  for (int f = 0; f < 4; f++) {
    const int p = shape_foot_prim(f);
    if (kw >= KIN_KW(prim_point) + 3 * p && kw < KIN_KW(prim_point) + 3 * p + 3) return SHAPE_FOOT_WORDS * f + kw - (KIN_KW(prim_point) + 3 * p);
    if (kw >= KIN_KW(prim_vel) + 3 * p && kw < KIN_KW(prim_vel) + 3 * p + 3) return SHAPE_FOOT_WORDS * f + 3 + kw - (KIN_KW(prim_vel) + 3 * p);
    if (kw == KIN_KW(prim_force) + p) return SHAPE_FOOT_WORDS * f + 6;
  }
  return -1;
}
// the store functor of a KinRow that keeps the feet's words: put(slot, value)
template <typename PUT> SD auto shape_foot_store(PUT put) {
  return [put](int kw, double v) {
    const int k = shape_foot_slot(kw);
    if (k >= 0) put(k, v);
  };
}

// contact_mask bits of the robot's primitives other than the four foot primitives
template <int ROBOT> constexpr int shape_collision_bits() {
  int m = (1 << Robot<ROBOT>::MD.nprims) - 1;
  for (int f = 0; f < 4; f++) m &= ~(1 << shape_foot_prim(f));
  return m;
}

// One row.  ld(w): word w of the state row (STATE_SW offsets);  cmask: its contact_mask;  foot(k): word k of the feet's 28 words
// (shape_foot_slot);  mld(w) / mst(w, v): word w of the solorl_env_shape row (SHAPE_MW offsets; word SHAPE_MW(prev_contact) holds the
// two int32 members);  tst(k, v): terms_out[k];  ep(k, v): ep_out[k] += v;  a: the row's actions;  reward: the row's reward or nullptr;
// cmd: the row's own command (vx, vy, yaw rate: solorl_shape_reward_cmd) or nullptr = the one of P.
template <int ROBOT, typename LD, typename FT, typename MLD, typename MST, typename TST, typename EP>
SD void shape_row(LD ld, int cmask, FT foot, MLD mld, MST mst, TST tst, EP ep, const solorl_shape_params& P, double sim_dt, double dtc,
                  const float* a, bool done, float* reward, const double* cmd = nullptr) {
  constexpr int NQ = Robot<ROBOT>::NQ;
  int32_t iw[2];                                            // prev_contact, valid
  const double ints = mld(SHAPE_MW(prev_contact));
  __builtin_memcpy(iw, &ints, sizeof(iw));
  auto st_ints = [&](int32_t prev_contact, int32_t valid) {
    const int32_t v[2] = {prev_contact, valid};
    double w;
    __builtin_memcpy(&w, v, sizeof(w));
    mst(SHAPE_MW(prev_contact), w);
  };
  if (done) {                                               // the episode's sums go out, its memory is cleared
    ep(0, 1.0);
    static_for<SHAPE_TERMS>([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      tst(k, 0.0);
      ep(1 + k, mld(SHAPE_MW(ep_sum) + k));
      mst(SHAPE_MW(ep_sum) + k, 0.0);
    });
    static_for<4>([&](auto fc) { mst(SHAPE_MW(air_time) + decltype(fc)::value, 0.0); });
    st_ints(0, 0);
    return;
  }
  const bool valid = iw[1] != 0;
  auto nost = [](int, double) {};
  const KinRow<double, ROBOT, LD, decltype(nost)> base(ld, nost, cmask, false, sim_dt, 0.0);     // pos, v0, w0 and R0 as every KinRow has them
  const M3<double>& R = base.R0;
  const V3<double> vb = mk(dot(R.c0, base.v0), dot(R.c1, base.v0), dot(R.c2, base.v0));         // R0^T lin_vel
  const V3<double> wb = mk(dot(R.c0, base.w0), dot(R.c1, base.w0), dot(R.c2, base.w0));
  const V3<double> gb = mk(-R.c0.z, -R.c1.z, -R.c2.z);                                           // R0^T (0, 0, -1)
  double t[SHAPE_TERMS];
  t[0] = vb.z * vb.z;
  t[1] = wb.x * wb.x + wb.y * wb.y;
  t[2] = gb.x * gb.x + gb.y * gb.y;
  const double dh = base.pos.z - P.base_height_target;
  t[3] = dh * dh;
  double tq = 0.0, jv = 0.0, ja = 0.0, ar = 0.0, pw = 0.0;
  static_for<NQ>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    const double tau = ld(STATE_SW(tau) + j), qd = ld(STATE_SW(qd) + j), aj = (double)a[j];
    const double dq = (qd - mld(SHAPE_MW(prev_qd) + j)) / dtc, da = aj - mld(SHAPE_MW(prev_action) + j);
    tq += tau * tau;
    jv += qd * qd;
    ja += valid ? dq * dq : 0.0;
    ar += valid ? da * da : 0.0;
    pw += fabs(tau * qd);
    mst(SHAPE_MW(prev_action) + j, aj);
    mst(SHAPE_MW(prev_qd) + j, qd);
  });
  t[4] = tq; t[5] = jv; t[6] = ja; t[7] = ar; t[8] = pw;
  double slip = 0.0, clear = 0.0, force = 0.0, airt = 0.0;
  int32_t contact = 0;
  static_for<4>([&](auto fc) {
    constexpr int f = decltype(fc)::value, w0 = SHAPE_FOOT_WORDS * f;
    const bool c = (cmask >> shape_foot_prim(f)) & 1;
    const double ux = foot(w0 + 3), uy = foot(w0 + 4), sp2 = ux * ux + uy * uy;
    const double dz = foot(w0 + 2) - P.foot_clearance_target, over = foot(w0 + 6) - P.foot_force_max;
    slip += c ? sp2 : 0.0;
    clear += c ? 0.0 : dz * dz * sqrt(sp2);
    force += over > 0.0 ? over : 0.0;
    const double air = mld(SHAPE_MW(air_time) + f) + dtc;
    const bool first = valid && c && !((iw[0] >> f) & 1);
    airt += first ? air - P.air_time_target : 0.0;
    mst(SHAPE_MW(air_time) + f, c ? 0.0 : air);
    contact |= (int32_t)c << f;
  });
  t[9] = slip; t[10] = clear; t[11] = force; t[12] = airt;
  t[13] = (double)__builtin_popcount((unsigned)(cmask & shape_collision_bits<ROBOT>()));
  const double cx = cmd ? cmd[0] : P.cmd_lin_vel[0], cy = cmd ? cmd[1] : P.cmd_lin_vel[1], cz = cmd ? cmd[2] : P.cmd_yaw_rate;
  const double ex = vb.x - cx, ey = vb.y - cy, ez = wb.z - cz;
  t[14] = exp(-(ex * ex + ey * ey) / P.tracking_sigma);
  t[15] = exp(-(ez * ez) / P.tracking_sigma);
  double s = 0.0;
  static_for<SHAPE_TERMS>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const double wt = P.weight[k] * t[k];
    tst(k, t[k]);
    s += wt;
    mst(SHAPE_MW(ep_sum) + k, mld(SHAPE_MW(ep_sum) + k) + wt);
  });
  if (reward) *reward = (float)((double)*reward + s);
  st_ints(contact, 1);
}

// leg L's foot words of a row: a KinRow that keeps them through put(slot, value)
template <int ROBOT, int L, typename LD, typename PUT> SD void shape_leg(LD ld, int cmask, PUT put, double sim_dt) {
  auto st = shape_foot_store(put);
  KinRow<double, ROBOT, LD, decltype(st)> row(ld, st, cmask, false, sim_dt, 0.0);
  row.template part<1 + L>();
}

// one row given as plain memory (the host program): state row, memory row in place, terms [16] or nullptr, ep_out column i of [17][n]
template <int ROBOT> SD void env_shape_row(const double* in, double* mem, const float* a, bool done, float* reward, double* terms, double* ep,
                                            size_t n, size_t i, const solorl_shape_params& P, double sim_dt, double dtc, const double* cmd = nullptr) {
  int32_t cmask;
  __builtin_memcpy(&cmask, in + KIN_IN_MASK_WORD, sizeof(cmask));
  double feet[SHAPE_FEET_WORDS];
  auto ld = [&](int w) { return in[w]; };
  static_for<4>([&](auto lc) { shape_leg<ROBOT, decltype(lc)::value>(ld, cmask, [&](int k, double v) { feet[k] = v; }, sim_dt); });
  shape_row<ROBOT>(ld, cmask, [&](int k) { return feet[k]; }, [&](int w) { return mem[w]; }, [&](int w, double v) { mem[w] = v; },
                   [&](int k, double v) { if (terms) terms[k] = v; }, [&](int k, double v) { if (ep) ep[(size_t)k * n + i] += v; }, P, sim_dt, dtc, a, done, reward, cmd);
}

}  // namespace solo
