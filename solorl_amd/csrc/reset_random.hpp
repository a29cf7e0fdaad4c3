// reset_random.hpp -- the row arithmetic of solorl_randomize_reset (include/solorl.h, "Randomised initial states", which holds the draw
// table): the nine Philox blocks of ONE solorl_env_state row's episode, the turn of its base, the height that puts its lowest support
// point at the asked clearance, and the contact cache it drops.  All in fp64.
//
// Four pieces, each a function of the row through ld(word) / st(word, value) functors with compile-time word indices (LDS at immediate
// offsets on the device), as kinematics.hpp and reward_shape.hpp: reset_draw_block<B> (block b of the table: independent of every other
// block), reset_orient (the three angles the blocks 6, 7, 8 return), reset_zmin_store (the store functor a KinRow is instantiated with
// here: it keeps the minimum of prim_point[p][2] over the robot's primitives and drops every other word of solorl_env_kin, so the
// support points are KinRow's own, not restated) and reset_lift.  solorl_reset.hip spreads the blocks and then the robot's five parts
// over four wavefronts, one lane per row; tests/host/reset_random_main.cpp, compiled by g++ under SOLO_HOST_SHIM, calls reset_row, which
// runs them one after the other.  The draws and the lift round every product and sum on its own (the header says so and the tests
// compare bits), so contraction into an FMA is switched off for those functions.  No index is computed from a row's data.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kinematics.hpp"
#include "perturb.hpp"

#ifdef SOLO_HOST_SHIM
using std::fmax;
using std::fmin;
#endif
#if defined(__clang__)
#define RESET_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RESET_NO_CONTRACT
#endif

namespace solo {

// last counter word of this stream (the env's own stream uses 1, 2, 3, the kicks 4, the noise 5, the actuator draws 6, the commands 7)
constexpr unsigned RESET_STREAM = 8u;
constexpr int RESET_BLOCKS = 9;                 // q 0..2, qd 3..5, lin_vel + yaw 6, ang_vel + roll 7, pitch 8
constexpr unsigned RESET_BLOCK_STRIDE = 16u;    // block b of episode k is counter word 16 k + b
// the part of a row that is read, and with the contact cache the part that is written: pos .. qd (one segment), the 24 lambda_prev
// words and the 8-byte word that holds contact_mask (low half) and rng_counter
constexpr int RESET_HEAD_WORDS = STATE_SW(tau);                 // 37
constexpr int RESET_LAMBDA_WORDS = SOLORL_STATE_MAX_PRIMS;      // 24
constexpr int RESET_MASK_WORD = KIN_IN_MASK_WORD;               // 254
constexpr uint32_t RESET_MASK_KEEP = 0xFF000000u;               // contact_mask bits that are no primitive's
static_assert(RESET_HEAD_WORDS == 37 && STATE_SW(qd) + SOLORL_STATE_MAX_DOF == RESET_HEAD_WORDS && STATE_SW(pos) == 0, "the head: pos, quat, lin_vel, ang_vel, q, qd");
static_assert(offsetof(solorl_env_state, rng_counter) == offsetof(solorl_env_state, contact_mask) + 4, "contact_mask is the low half of its word");
static_assert(sizeof(solorl_reset_randomization) == 16 + 8 * (12 + 12 + 3 + 3 + 4) + 8, "struct of include/solorl.h");

struct ResetAngles { double yaw, roll, pitch; };     // psi, phi, theta of the table; 0 where the half-width is 0

// neither NaN nor +-Inf, by comparisons alone
PERTURB_HD bool reset_finite(double x) { return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; }

// block b of episode k of env gid
PERTURB_HD void reset_block(const solorl_reset_randomization& P, long long gid, unsigned k, unsigned b, unsigned (&out)[4]) {
  perturb_philox((unsigned)P.seed, (unsigned)(P.seed >> 32), (unsigned)gid, (unsigned)((unsigned long long)gid >> 32), RESET_BLOCK_STRIDE * k + b, RESET_STREAM, out);
}
// d = (2u - 1) a with u = (word >> 8) 2^-24: 2u - 1 is exact, the product rounds once
PERTURB_HD double reset_delta(unsigned word, double a) {
  RESET_NO_CONTRACT
  const double u = (double)(word >> 8) * (1.0 / 16777216.0);
  const double s = 2.0 * u - 1.0;
  return s * a;
}
// member + d: the second rounding
PERTURB_HD double reset_add(double x, unsigned word, double a) {
  RESET_NO_CONTRACT
  const double d = reset_delta(word, a);
  return x + d;
}
PERTURB_HD double reset_clamp(double x, double lim) { return fmin(fmax(x, -lim), lim); }
// pos.z + (clearance - zmin)
PERTURB_HD double reset_lift(double z, double clearance, double zmin) {
  RESET_NO_CONTRACT
  const double up = clearance - zmin;
  return z + up;
}

// whether the base is turned at all, and whether the pose can change (then the contact cache is dropped)
PERTURB_HD bool reset_turns(const solorl_reset_randomization& P) { return P.yaw != 0.0 || P.roll != 0.0 || P.pitch != 0.0; }
template <int ROBOT> PERTURB_HD bool reset_pose_changes(const solorl_reset_randomization& P) {
  bool any = reset_turns(P) || P.place_on_ground != 0;
  for (int j = 0; j < (ROBOT ? 12 : 8); j++) any = any || P.joint_pos[j] != 0.0;
  return any;
}

// Block B of the table on one row.  ld(w) / st(w, v): word w of the state row (STATE_SW offsets, all within the head).  The angle a
// block draws goes into A.  A block whose half-widths are all 0 draws nothing.
template <int ROBOT, int B, typename LD, typename ST>
SD void reset_draw_block(LD ld, ST st, const solorl_reset_randomization& P, double joint_limit, long long gid, unsigned k, ResetAngles& A) {
  static_assert(B >= 0 && B < RESET_BLOCKS, "nine blocks");
  constexpr int NQ = Robot<ROBOT>::NQ;
  unsigned r[4];
  if constexpr (B < 6) {
    constexpr bool VEL = B >= 3;
    constexpr int j0 = 4 * (B % 3), W0 = VEL ? STATE_SW(qd) : STATE_SW(q);
    if constexpr (j0 < NQ) {                        // (a Solo8 has no joints 8..11: blocks 2 and 5 are not drawn)
      const double* a = VEL ? P.joint_vel : P.joint_pos;
      if (a[j0] == 0.0 && a[j0 + 1] == 0.0 && a[j0 + 2] == 0.0 && a[j0 + 3] == 0.0) return;
      reset_block(P, gid, k, (unsigned)B, r);
      static_for<4>([&](auto wc) {
        constexpr int w = decltype(wc)::value, j = j0 + w;
        if (a[j] != 0.0) {
          const double x = reset_add(ld(W0 + j), r[w], a[j]);
          st(W0 + j, VEL ? x : reset_clamp(x, joint_limit));
        }
      });
    }
  } else {
    const double* a = B == 6 ? P.lin_vel : P.ang_vel;
    const double turn = B == 6 ? P.yaw : B == 7 ? P.roll : P.pitch;
    constexpr int W0 = B == 6 ? STATE_SW(lin_vel) : STATE_SW(ang_vel);
    const bool vel = B < 8 && (a[0] != 0.0 || a[1] != 0.0 || a[2] != 0.0);
    if (!vel && turn == 0.0) return;
    reset_block(P, gid, k, (unsigned)B, r);
    if constexpr (B < 8) static_for<3>([&](auto wc) {
      constexpr int w = decltype(wc)::value;
      if (a[w] != 0.0) st(W0 + w, reset_add(ld(W0 + w), r[w], a[w]));
    });
    const double angle = turn == 0.0 ? 0.0 : reset_delta(r[B < 8 ? 3 : 0], turn);
    if constexpr (B == 6) A.yaw = angle;
    else if constexpr (B == 7) A.roll = angle;
    else A.pitch = angle;
  }
}

// quat <- Rz(yaw) quat Rx(roll) Ry(pitch), normalised, w >= 0
template <typename LD, typename ST> SD void reset_orient(LD ld, ST st, const ResetAngles& A) {
  const SinCos<double> y = sincos_call(A.yaw * 0.5), r = sincos_call(A.roll * 0.5), p = sincos_call(A.pitch * 0.5);
  const Quat<double> q{ld(STATE_SW(quat)), ld(STATE_SW(quat) + 1), ld(STATE_SW(quat) + 2), ld(STATE_SW(quat) + 3)};
  const Quat<double> z{y.c * q.x - y.s * q.y, y.c * q.y + y.s * q.x, y.c * q.z + y.s * q.w, y.c * q.w - y.s * q.z};      // (0, 0, s, c) (x) q
  const Quat<double> o = quat_rot_axis<1>(quat_rot_axis<0>(z, r.c, r.s), p.c, p.s);
  const double inv = 1.0 / sqrt(o.x * o.x + o.y * o.y + o.z * o.z + o.w * o.w);
  const double n = o.w < 0.0 ? -inv : inv;
  st(STATE_SW(quat), o.x * n); st(STATE_SW(quat) + 1, o.y * n); st(STATE_SW(quat) + 2, o.z * n); st(STATE_SW(quat) + 3, o.w * n);
}

// word kw of solorl_env_kin is the z of a support point of a primitive this robot has
template <int ROBOT> SD constexpr bool reset_is_support_z(int kw) {
  const int k = kw - KIN_KW(prim_point);
  return k >= 0 && k < 3 * Robot<ROBOT>::MD.nprims && k % 3 == 2;
}
// the store functor of a KinRow that keeps the smallest support z in zmin (a NaN point is skipped: fmin's rule)
template <int ROBOT> SD auto reset_zmin_store(double& zmin) {
  return [&zmin](int kw, double v) {
    if (reset_is_support_z<ROBOT>(kw)) zmin = fmin(zmin, v);
  };
}
// a reader of a row of which only the head is at hand (the words a KinRow asks for beyond it feed members the store drops)
template <typename LD> SD auto reset_head_reader(LD ld) {
  return [ld](int w) { return w < RESET_HEAD_WORDS ? ld(w) : 0.0; };
}
// the smallest support z of part PART (0 the base's twelve points, 1 + L leg L) of the row
template <int ROBOT, int PART, typename LD> SD double reset_part_zmin(LD ld) {
  double zmin = __builtin_inf();
  auto st = reset_zmin_store<ROBOT>(zmin);
  auto rd = reset_head_reader(ld);
  KinRow<double, ROBOT, decltype(rd), decltype(st)> row(rd, st, 0, false, 1.0, 0.0);
  row.template part<PART>();
  return zmin;
}

// the contact cache of a row given as plain memory
SD void reset_clear_contacts(double* row) {
  for (int p = 0; p < RESET_LAMBDA_WORDS; p++) row[STATE_SW(lambda_prev) + p] = 0.0;
  uint32_t m[2];
  __builtin_memcpy(m, row + RESET_MASK_WORD, sizeof(m));
  m[0] &= RESET_MASK_KEEP;
  __builtin_memcpy(row + RESET_MASK_WORD, m, sizeof(m));
}

// one LIVE row given as plain memory (the host program), env gid, its count word in/out
template <int ROBOT> SD void reset_row(double* row, uint32_t* count, const solorl_reset_randomization& P, double joint_limit, long long gid) {
  const unsigned k = *count;
  auto ld = [row](int w) { return row[w]; };
  auto st = [row](int w, double v) { row[w] = v; };
  ResetAngles A{0.0, 0.0, 0.0};
  static_for<RESET_BLOCKS>([&](auto bc) { reset_draw_block<ROBOT, decltype(bc)::value>(ld, st, P, joint_limit, gid, k, A); });
  if (reset_turns(P)) reset_orient(ld, st, A);
  if (P.place_on_ground != 0) {
    double zmin = __builtin_inf();
    static_for<KIN_PARTS>([&](auto pc) { zmin = fmin(zmin, reset_part_zmin<ROBOT, decltype(pc)::value>(ld)); });
    st(STATE_SW(pos) + 2, reset_lift(ld(STATE_SW(pos) + 2), P.clearance, zmin));
  }
  if (reset_pose_changes<ROBOT>(P)) reset_clear_contacts(row);
  *count = k + 1u;
}

// why the entry point refuses *p with this joint_limit, or nullptr.  Host only (the entry point and the host program).
inline const char* reset_refusal(const solorl_reset_randomization& P, double joint_limit) {
  constexpr double PI = 3.14159265358979323846;
  auto width = [](double a) { return reset_finite(a) && a >= 0.0; };
  for (int j = 0; j < 12; j++)
    if (!width(P.joint_pos[j]) || !width(P.joint_vel[j])) return "joint_pos and joint_vel half-widths must be finite and >= 0";
  for (int k = 0; k < 3; k++)
    if (!width(P.lin_vel[k]) || !width(P.ang_vel[k])) return "lin_vel and ang_vel half-widths must be finite and >= 0";
  if (!width(P.yaw) || !width(P.roll) || !width(P.pitch)) return "yaw, roll and pitch half-widths must be finite and >= 0";
  if (P.yaw > PI || P.roll > PI || P.pitch > PI) return "yaw, roll and pitch half-widths must not exceed pi";
  if (!width(P.clearance)) return "clearance must be finite and >= 0";
  if (!width(joint_limit)) return "cfg joint_limit must be finite and >= 0";
  return nullptr;
}

}  // namespace solo
