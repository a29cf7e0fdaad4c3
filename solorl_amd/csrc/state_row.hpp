// state_row.hpp -- what a reader of ONE solorl_env_state row needs, whatever it derives from the row (kinematics.hpp, dyn_tensors.hpp):
// the row's size and member offsets in 8-byte words, the scheduling fence between a row's independent outputs, sin and cos by a call,
// and the K2 inertia entries of a link.
#pragma once
#include <cstddef>

#include "dynamics.hpp"

namespace solo {

constexpr int STATE_WORDS = sizeof(solorl_env_state) / 8;         // 255
constexpr int KIN_STATE_WORDS = STATE_WORDS;                       // its name while kinematics.hpp held it: host programs written then still build
static_assert(sizeof(solorl_env_state) == 2040 && offsetof(solorl_env_state, pos) == 0, "row size of include/solorl.h, in whole 8-byte words");

#define STATE_SW(member) ((int)(offsetof(solorl_env_state, member) / 8))

// After every link, primitive and row of a matrix: no instruction is scheduled across.  A row's outputs are stores nothing waits for and
// the links' chains are independent, so left alone the scheduler computes far ahead of the stores: the kernel went to 512 registers and
// spilled.
#ifdef SOLO_HOST_SHIM
#define ROW_FENCE() do {} while (0)
#else
#define ROW_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif

// sin and cos by a CALL: a row needs them for every joint angle (and its half), and the fp64 routine with its argument reduction is
// several hundred instructions -- inlined two dozen times it was most of the kernel
template <typename T> struct SinCos { T s, c; };
template <typename T> SNI SinCos<T> sincos_call(T x) {
  SinCos<T> r;
  sincos_t(x, r.s, r.c);
  return r;
}

// K2 inertia of link l about its COM in link axes: Bullet's box rule (diagonal) or the URDF tensor
template <typename T> struct LinkInertia { T xx, yy, zz, xy, xz, yz; };
template <typename T, int ROBOT, int l> SD LinkInertia<T> link_inertia(bool urdf) {
  constexpr solorl_link_data LK = Robot<ROBOT>::MD.links[l];
  return {urdf ? T(LK.inertia_urdf[0]) : T(LK.inertia_box[0]), urdf ? T(LK.inertia_urdf[1]) : T(LK.inertia_box[1]),
          urdf ? T(LK.inertia_urdf[2]) : T(LK.inertia_box[2]), urdf ? T(LK.inertia_urdf[3]) : T(0), urdf ? T(LK.inertia_urdf[4]) : T(0),
          urdf ? T(LK.inertia_urdf[5]) : T(0)};
}

}  // namespace solo
