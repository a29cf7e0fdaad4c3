// k7_gate_share.cpp -- DEV TOOL (tools/dev/k7_gate_share.py builds and drives it; nothing in solorl_amd/ can call it).
// One fp32 physics sub-step through the kernel's lane-mode code path on the CPU, as tests/host/host_harness.cpp runs it, with
// phase_pgs' per-sweep hook switched on: the lane-mode row loop has the rows, the order, the cone projection and the K7 rule of the
// team sweep, so what it sees per sweep is what a team of pgs_team_variant sees.  Recorded per solve: the contacts, the sweeps run,
// and a bit per sweep in which NO limit or normal row changed by more than its threshold -- the sweeps in which a gated team sweep
// has to form the friction pairs' residual entries (its cold block).
#define SOLO_HOST_SHIM 1
#include <cstdint>
#include <cstring>
#include <vector>
struct K7Solve { int nc, nlim, sweeps; uint64_t quiet_ln; };
static K7Solve k7_cur;
// (an env that is finished sweeps no more in lane mode either: the hook only sees sweeps of an unfinished solve)
#define SOLO_K7_SWEEP_HOOK(nlim_, nc_, viol_ln_, viol_) do { \
    k7_cur.nlim = (nlim_); k7_cur.nc = (nc_); \
    if (!(viol_ln_)) k7_cur.quiet_ln |= 1ull << k7_cur.sweeps; \
    k7_cur.sweeps++; } while (0)
#include "../../tests/host/host_shim.hpp"
#include "../../include/solorl.h"
#include "../../solorl_amd/csrc/dynamics.hpp"
using namespace solo;

// (the state <-> context plumbing of host_harness.cpp, fp32 Solo12 only)
extern "C" void k7_substep(solorl_env_state* s, const solorl_config* c, int* nc, int* nlim, int* sweeps, uint64_t* quiet_ln) {
  using T = float;
  constexpr int ROBOT = 1;
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
  for (int j = 0; j < NQ; j++) { st.q[j] = (T)s->q[j]; st.qd[j] = (T)s->qd[j]; C.tau[j] = (T)s->tau[j]; }
  for (int p = 0; p < NPRIM; p++) lam[p] = (T)s->lambda_prev[p];
  k7_cur = K7Solve{0, 0, 0, 0};
  int mask = substep<T, ROBOT>(C, pp, lam, 1, lds);
  *nc = k7_cur.nc; *nlim = k7_cur.nlim; *sweeps = k7_cur.sweeps; *quiet_ln = k7_cur.quiet_ln;
  s->pos[0] = st.pos.x; s->pos[1] = st.pos.y; s->pos[2] = st.pos.z;
  s->quat[0] = st.qx; s->quat[1] = st.qy; s->quat[2] = st.qz; s->quat[3] = st.qw;
  s->lin_vel[0] = st.v.x; s->lin_vel[1] = st.v.y; s->lin_vel[2] = st.v.z;
  s->ang_vel[0] = st.w.x; s->ang_vel[1] = st.w.y; s->ang_vel[2] = st.w.z;
  for (int j = 0; j < NQ; j++) { s->q[j] = st.q[j]; s->qd[j] = st.qd[j]; if (!c->hold_torque) s->tau[j] = 0; }
  for (int p = 0; p < NPRIM; p++) s->lambda_prev[p] = lam[p];
  s->contact_mask = mask;
}
