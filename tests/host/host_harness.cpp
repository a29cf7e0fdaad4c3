// host_harness.cpp -- TEST ONLY.  One physics sub-step through the *kernel's* templated code path
// (dynamics.hpp) on the CPU, one lane, T = float or double.
#define SOLO_HOST_SHIM 1
#include <cstring>
#include <vector>
#include "../../include/solorl.h"
#include "../../solorl_amd/csrc/dynamics.hpp"
using namespace solo;

template <typename T, int ROBOT>
static void run(solorl_env_state* s, const solorl_config* c, int apply_tau) {
  using RB = Robot<ROBOT>;
  constexpr int NQ = RB::NQ;
  std::vector<unsigned char> mem(RowLds<T>::bytes(1) + 64);
  RowLds<T> lds; lds.lanes = 1; lds.lane = 0; lds.base = mem.data();
  const PhysParams<T> pp = make_phys<T>(*c);
  SubCtx<T, ROBOT> C;
  PhysState<T, NQ>& st = C.ps;
  C.tmy = (T)s->treadmill_y;
  st.pos = mk((T)s->pos[0], (T)s->pos[1], (T)s->pos[2]);
  st.qx = (T)s->quat[0]; st.qy = (T)s->quat[1]; st.qz = (T)s->quat[2]; st.qw = (T)s->quat[3];
  st.v = mk((T)s->lin_vel[0], (T)s->lin_vel[1], (T)s->lin_vel[2]);
  st.w = mk((T)s->ang_vel[0], (T)s->ang_vel[1], (T)s->ang_vel[2]);
  T lam[NPRIM];
  for (int j = 0; j < NQ; j++) { st.q[j] = (T)s->q[j]; st.qd[j] = (T)s->qd[j]; C.tau[j] = apply_tau ? (T)s->tau[j] : T(0); }
  for (int p = 0; p < NPRIM; p++) lam[p] = (T)s->lambda_prev[p];
  int mask = substep<T, ROBOT>(C, pp, lam, 1, lds);
  s->pos[0] = st.pos.x; s->pos[1] = st.pos.y; s->pos[2] = st.pos.z;
  s->quat[0] = st.qx; s->quat[1] = st.qy; s->quat[2] = st.qz; s->quat[3] = st.qw;
  s->lin_vel[0] = st.v.x; s->lin_vel[1] = st.v.y; s->lin_vel[2] = st.v.z;
  s->ang_vel[0] = st.w.x; s->ang_vel[1] = st.w.y; s->ang_vel[2] = st.w.z;
  for (int j = 0; j < NQ; j++) { s->q[j] = st.q[j]; s->qd[j] = st.qd[j]; if (!c->hold_torque) s->tau[j] = 0; }
  for (int p = 0; p < NPRIM; p++) s->lambda_prev[p] = lam[p];
  s->contact_mask = mask;
}

// HARNESS_ONLY_ROBOT and HARNESS_ONLY_FLOAT (0 or 1 each; both or neither): build one of the four instantiations only -- a sanitizer build of all four in
// one translation unit takes minutes (tests/host/nonfinite_main.cpp builds them side by side); the others then do nothing.
#if defined(HARNESS_ONLY_ROBOT) != defined(HARNESS_ONLY_FLOAT)
#error "HARNESS_ONLY_ROBOT and HARNESS_ONLY_FLOAT come as a pair"
#endif
#ifdef HARNESS_ONLY_ROBOT
#define HARNESS_RUN(T, R, F) do { if ((R) == HARNESS_ONLY_ROBOT && (F) == HARNESS_ONLY_FLOAT) run<T, HARNESS_ONLY_ROBOT>(s, c, 1); } while (0)
#else
#define HARNESS_RUN(T, R, F) run<T, R>(s, c, 1)
#endif
extern "C" void harness_substep(solorl_env_state* s, const solorl_config* c, int use_float) {
#if !defined(HARNESS_ONLY_FLOAT) || HARNESS_ONLY_FLOAT == 1
  if (use_float) { if (c->robot == SOLORL_ROBOT_SOLO12) HARNESS_RUN(float, 1, 1); else HARNESS_RUN(float, 0, 1); }
#endif
#if !defined(HARNESS_ONLY_FLOAT) || HARNESS_ONLY_FLOAT == 0
  if (!use_float) { if (c->robot == SOLORL_ROBOT_SOLO12) HARNESS_RUN(double, 1, 0); else HARNESS_RUN(double, 0, 0); }
#endif
}
