// solorl_hip.hip -- gfx950 kernels + the C ABI of include/solorl.h.
//
// Hot path: one launch of `step_kernel` = SoloBaseEnv.step for every env
// (reference baseEnv.py:42-68) INCLUDING the worker's auto-reset (agents/ppo/envs.py:38-40):
//   A3 apply_action (solo.py:224-259, controllers/PD.py:3-10)  -> A4 simulator_step (solo.py:261-274:
//   history push, frame_skip x physics sub-step, pointgoal progress) -> A6 observation
//   (solo.py:186-222) -> A7 reward (baseEnv.py:91-157) -> A8 termination (baseEnv.py:162-180)
//   -> A1 terminal reward override / info (baseEnv.py:52-66) -> A2/A9 reset (baseEnv.py:70-82).
//
// Layout: struct-of-arrays state in HBM (field-major).  Team mode (default): 16 lanes per env, 4 envs per
// wavefront, per-env context and constraint rows in LDS, the PGS sweep register-resident (dynamics.hpp).
// Lane mode (SOLORL_TEAM=0): one env per lane, 64 envs per workgroup, rows in LDS, the rest in VGPRs.
//
// Reset is O(1): `reset = fixed pose + K zero-torque control steps` is a pure function of K
// (5..11), so the post-settle states are simulated ONCE at create time by this same kernel
// (mode = SETTLE) into a snapshot table and a terminating lane just loads snapshot[K].
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <string>
#include <vector>

#include "../../include/solorl.h"
#include "dynamics.hpp"
#include "perturb.hpp"

using namespace solo;

#ifndef SOLO_TU_PART
#define SOLO_TU_PART -1      // translation-unit split, see dispatch_step below
#endif
// the thread-local error message lives in the part that holds the C ABI; the other parts (and solorl_ppo.hip) report through it
extern "C" __attribute__((visibility("hidden"))) int solorl_fail_(int code, const char* msg);

namespace {

#if SOLO_TU_PART == -1 || SOLO_TU_PART == 4
thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
#else
int fail(int code, const std::string& msg) { return solorl_fail_(code, msg.c_str()); }
#endif
#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(SOLORL_ERR_HIP, std::string(#x ": ") + hipGetErrorString(e_)); } while (0)

constexpr int DMAX = SOLORL_STATE_MAX_OBS;   // 42
constexpr int HSTRIDE = (DMAX + 3) & ~3;     // fields per history level in the state storage: 44 (whole 64-B sectors, see SX)
using idx_t = unsigned;   // device-side element indices: 32-bit (solorl_create checks NF*N and O*N < 2^31); 64-bit index
                          // arithmetic made every state access ~10 VALU instructions

// field-major state layout (offsets in units of N elements)
struct Layout {
  int n, D, H, NF;
  int pos, quat, v, w, q, qd, lam, hist, goal, pot, prog, goals, egoals, dr, xyprev, tmy;
};
enum { I_TIMESTEP = 0, I_MASK = 1, I_RNG = 2, I_NEEDRESET = 3, I_ENVID = 4, NI = 5 };   // I_ENVID: slot -> env id

// State storage, "AoSoA-4": slots are grouped in fours (= the four envs of a team-mode wavefront) and a group holds its
// fields as [field][4], so a group is one contiguous block of NF x 16 B.  The team's lanes (field t, t+16, ... of slot
// e & 3) then read and write whole 64-B sectors: 4 sectors per wave instruction where the field-major layout of round 1
// touched 16, and its 16-B partial writes were counted (and paid for) as full 64-B write requests -- 11.0 MB of HBM writes
// per launch against 3.2 MB of bytes actually stored.  Snapshots use the same indexing over their own slot count.
SD idx_t SX(int f, idx_t e, int nf) { return (e >> 2) * (idx_t)(nf << 2) + ((idx_t)f << 2) + (e & 3u); }

Layout make_layout(int n, int D, int H) {
  Layout L; int o = 0;
  L.n = n; L.D = D; L.H = H;
  // every block starts on a multiple of 4 fields = a 64-B sector of the group (SX), and NF is one, so groups are sector-aligned
  auto align4 = [&]() { o = (o + 3) & ~3; };
  L.pos = o; o += 3; L.quat = o; o += 4; L.v = o; o += 3; L.w = o; o += 3;
  L.q = o; o += n; L.qd = o; o += n; align4(); L.lam = o; o += NPRIM; align4(); L.hist = o; o += (H > 2 ? H : 2) * HSTRIDE; align4();      // (levels 0 and 1 always have their place; deeper ones only when asked for)
  L.goal = o; o += 2; L.pot = o++; L.prog = o++; L.goals = o++; L.egoals = o++; L.dr = o; o += 5; L.xyprev = o; o += 2; L.tmy = o++;
  align4();
  L.NF = o;
  return L;
}

struct EnvParams {
  int task, control, frame_skip, episode_length, hold_torque, disable_termination;
  int settle_min, nsettle;
  int use_treadmill; float tm_offset;         // treadmill: side redrawn at reset (simulation.py:72-74)
  int linear_ids;                             // slot e holds env e (no contact-count sorting): no slot -> env-id load on the step's critical path
  int lds_poison_on; unsigned lds_poison;     // test hook, see step_body
  unsigned seed_lo, seed_hi; long long id0;
  double kp, kd, max_torque, reward_dt;
  const double* dyn;     // device block of the handle's MUTABLE parameters ([0] = goal_radius): a by-value copy would be frozen
                         // into a captured HIP graph (solorl_increment_curriculum between replays must be seen)
};
enum { DYN_GOAL_RADIUS = 0, NDYN = 4 };

enum { MODE_STEP = 0, MODE_SETTLE = 1 };

// solorl_step_act: Policy.act on the observation a step has just written, by the wavefront that wrote it (policy_tail_team)
struct PolicyTail {
  const float *cw0, *cb0, *cw1, *cb1, *cw2, *cb2, *aw0, *ab0, *aw1, *ab1, *mw, *mb, *logstd;
  const float* noise;                       // [N][A] standard-normal draw, or null (action = mean)
  float *value, *action, *logp;             // [N], [N][A], [N]; value == null: no policy tail in this launch
};

struct Outputs {
  float* obs; float* rew; unsigned char* done;
  unsigned char *timeout, *success, *nan_reset; int* ep_len; float *ep_rew, *goals, *dr0, *dr1, *dr2, *dr3, *dr4;
  float* ep_stats;     // [SOLORL_EPSTAT_FIELDS][N] finished-episode accumulators (include/solorl.h), or null
  float* tau;          // [N][A] applied joint torques of this step (include/solorl.h applied_torque), or null
  PolicyTail pol;
};

// ---------------------------------------------------------------- device helpers
SD void philox(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Bullet getEulerZYX (K10), as returned by p.getEulerFromQuaternion: roll, pitch, yaw
template <typename T> SD void euler_zyx(T x, T y, T z, T w, T& roll, T& pitch, T& yaw) {
  T sqx = x * x, sqy = y * y, sqz = z * z, squ = w * w;
  T sarg = T(-2) * (x * z - w * y);
  if (sarg <= T(-0.99999)) { pitch = T(-0.5 * M_PI); roll = T(0); yaw = T(2) * atan2(x, -y); }
  else if (sarg >= T(0.99999)) { pitch = T(0.5 * M_PI); roll = T(0); yaw = T(2) * atan2(-x, y); }
  else {
    pitch = asin(sarg);
    roll = atan2(T(2) * (y * z + w * x), squ - sqx - sqy + sqz);
    yaw = atan2(T(2) * (x * y + w * z), squ + sqx - sqy - sqz);
  }
}

template <typename T, int NQ> struct Env {
  PhysState<T, NQ> ps;
  T goal[2], pot, prog, goals, egoals, dr[5], xyprev[2], tmy;
  int timestep, mask, rng;
};

template <typename T, int NQ>
SD void load_env(Env<T, NQ>& E, const T* sf, const int* si, const Layout& L, idx_t N, idx_t e) {
  auto F = [&](int f) { return sf[SX(f, e, L.NF)]; };
  E.ps.pos = mk(F(L.pos), F(L.pos + 1), F(L.pos + 2));
  E.ps.qx = F(L.quat); E.ps.qy = F(L.quat + 1); E.ps.qz = F(L.quat + 2); E.ps.qw = F(L.quat + 3);
  E.ps.v = mk(F(L.v), F(L.v + 1), F(L.v + 2)); E.ps.w = mk(F(L.w), F(L.w + 1), F(L.w + 2));
#pragma unroll
  for (int j = 0; j < NQ; j++) { E.ps.q[j] = F(L.q + j); E.ps.qd[j] = F(L.qd + j); }
  E.goal[0] = F(L.goal); E.goal[1] = F(L.goal + 1); E.pot = F(L.pot); E.prog = F(L.prog);
  E.goals = F(L.goals); E.egoals = F(L.egoals);
#pragma unroll
  for (int k = 0; k < 5; k++) E.dr[k] = F(L.dr + k);
  E.xyprev[0] = F(L.xyprev); E.xyprev[1] = F(L.xyprev + 1); E.tmy = F(L.tmy);
  E.timestep = si[SX(I_TIMESTEP, e, NI)]; E.mask = si[SX(I_MASK, e, NI)]; E.rng = si[SX(I_RNG, e, NI)];
}
template <typename T, int NQ>
SD void store_env(const Env<T, NQ>& E, T* sf, int* si, const Layout& L, idx_t N, idx_t e) {
  auto F = [&](int f, T v) { sf[SX(f, e, L.NF)] = v; };
  F(L.pos, E.ps.pos.x); F(L.pos + 1, E.ps.pos.y); F(L.pos + 2, E.ps.pos.z);
  F(L.quat, E.ps.qx); F(L.quat + 1, E.ps.qy); F(L.quat + 2, E.ps.qz); F(L.quat + 3, E.ps.qw);
  F(L.v, E.ps.v.x); F(L.v + 1, E.ps.v.y); F(L.v + 2, E.ps.v.z);
  F(L.w, E.ps.w.x); F(L.w + 1, E.ps.w.y); F(L.w + 2, E.ps.w.z);
#pragma unroll
  for (int j = 0; j < NQ; j++) { F(L.q + j, E.ps.q[j]); F(L.qd + j, E.ps.qd[j]); }
  F(L.goal, E.goal[0]); F(L.goal + 1, E.goal[1]); F(L.pot, E.pot); F(L.prog, E.prog);
  F(L.goals, E.goals); F(L.egoals, E.egoals);
#pragma unroll
  for (int k = 0; k < 5; k++) F(L.dr + k, E.dr[k]);
  F(L.xyprev, E.xyprev[0]); F(L.xyprev + 1, E.xyprev[1]); F(L.tmy, E.tmy);
  si[SX(I_TIMESTEP, e, NI)] = E.timestep; si[SX(I_MASK, e, NI)] = E.mask; si[SX(I_RNG, e, NI)] = E.rng;
}

// SoloBase.get_current_state (solo.py:198-222): D values, compile-time indices
template <typename T, int ROBOT>
SD void current_state(const Env<T, Robot<ROBOT>::NQ>& E, int task, T (&cs)[DMAX]) {
  constexpr int NQ = Robot<ROBOT>::NQ;
  T r, p, y;
  euler_zyx(E.ps.qx, E.ps.qy, E.ps.qz, E.ps.qw, r, p, y);
  cs[0] = E.ps.pos.z;
  cs[1] = (r - T(2) * floor(r * T(0.5))) * T(0.5);   // (euler % 2*pi)/(2*pi) == (euler % 2)/2, solo.py:206
  cs[2] = (p - T(2) * floor(p * T(0.5))) * T(0.5);
  cs[3] = (y - T(2) * floor(y * T(0.5))) * T(0.5);
  cs[4] = E.ps.v.x; cs[5] = E.ps.v.y; cs[6] = E.ps.v.z;
  cs[7] = E.ps.w.x; cs[8] = E.ps.w.y; cs[9] = E.ps.w.z;
#pragma unroll
  for (int j = 0; j < NQ; j++) { cs[10 + j] = E.ps.q[j] * T(0.1); cs[10 + NQ + j] = E.ps.qd[j] * T(0.01); }   // (/10, /100: solo.py:208-209)
#pragma unroll
  for (int f = 0; f < 4; f++)    // solo.py:310-323: contacts with the plane body, which also lies under the treadmill strip -- a foot
    cs[10 + 2 * NQ + f] = ((E.mask >> (13 + 2 * f)) & 1) ? T(1) : T(0);     // over the strip (bit 24+f) is reported like any other
  if (task == SOLORL_TASK_POINTGOAL) {
    cs[14 + 2 * NQ] = E.ps.pos.x * T(0.5); cs[15 + 2 * NQ] = E.ps.pos.y * T(0.5);
    cs[16 + 2 * NQ] = E.goal[0] * T(0.5); cs[17 + 2 * NQ] = E.goal[1] * T(0.5);
  }
}

template <typename T, int NQ>
SD void sample_goal(Env<T, NQ>& E, const EnvParams& P, long long gid) {   // solo.py:325-330
  unsigned r[4];
  philox(P.seed_lo, P.seed_hi, (unsigned)gid, (unsigned)((unsigned long long)gid >> 32), (unsigned)E.rng++, 1u, r);
  T span = T(P.dyn[DYN_GOAL_RADIUS] - 1.0);
  T x = T(1) + T((double)(r[0] >> 8) * (1.0 / 16777216.0)) * span;
  T y = T(1) + T((double)(r[1] >> 8) * (1.0 / 16777216.0)) * span;
  E.goal[0] = (r[2] & 1u) ? x : -x; E.goal[1] = (r[3] & 1u) ? y : -y;
}

// ---- the scalar env logic of a control step: one copy, run by lane mode's lane (step_body) and by team mode's leader (step_team)
template <typename T, int NQ>
SD void pointgoal_progress(Env<T, NQ>& E, const EnvParams& P, long long gid) {   // solo.py:266-272
  T dx = E.ps.pos.x - E.goal[0], dy = E.ps.pos.y - E.goal[1];
  T np = sqrt(dx * dx + dy * dy);
  E.prog = -(np - E.pot); E.pot = np;
  if (np < T(0.5)) { E.goals += T(1); sample_goal(E, P, gid); }
}
// A7 reward, NaN guard, A8 termination, A1 terminal reward override, every per-env output and the ep_stats accumulators; returns done.
// asq: sum of the raw action squares; N: envs of the launch (the ep_stats column stride)
template <typename T, int NQ>
SD int reward_termination_outputs(Env<T, NQ>& E, const EnvParams& P, T asq, const Outputs& out, idx_t env, int N) {
  // ---- A7 reward (baseEnv.py:91-157)
  const T z = E.ps.pos.z;
  T stand = z > T(0.2) ? T(0.5) : T(0), jp = T(0), balance = T(0), progress = T(0), torque = T(0);
#pragma unroll
  for (int j = 0; j < NQ; j++) jp += P.task == SOLORL_TASK_STAND ? fabs(E.ps.q[j]) : E.ps.q[j] * E.ps.q[j];
  jp = T(-0.1) * jp / T(NQ);
  if (P.task == SOLORL_TASK_WALK) {
    if (z > T(0.2)) { T vx = E.ps.v.x; progress = T(2) * (vx > T(0) ? T(1) : (vx < T(0) ? T(-1) : T(0))) * vx * vx; }
  } else if (P.task == SOLORL_TASK_POINTGOAL) {
    T r, p, y; euler_zyx(E.ps.qx, E.ps.qy, E.ps.qz, E.ps.qw, r, p, y);
    balance = T(-0.1) * (fabs(r) + fabs(p));
    if (z > T(0.2)) progress = E.prog * T(1.0 / P.reward_dt);
  }
  if (P.control == SOLORL_CONTROL_TORQUE) torque = T(-0.01) * asq;
  T reward = stand + jp + balance + progress + torque;
  E.dr[0] += stand; E.dr[1] += jp; E.dr[2] += torque; E.dr[3] += balance; E.dr[4] += progress;

  // ---- A8 termination (baseEnv.py:162-180) + NaN guard
  int done = 0, to = 0, su = 0, nanr = 0;
  {
    T chk = E.ps.pos.x + E.ps.pos.y + E.ps.pos.z + E.ps.qw + E.ps.v.x + E.ps.v.y + E.ps.v.z + E.ps.w.x + E.ps.w.y + E.ps.w.z;
#pragma unroll
    for (int j = 0; j < NQ; j++) chk += E.ps.q[j] + E.ps.qd[j];
    if (!(fabs(chk) < T(1e30))) { nanr = 1; done = 1; reward = T(0); }
  }
  if (!P.disable_termination && !nanr) {
    if (E.timestep >= P.episode_length) { done = 1; to = 1; su = P.task != SOLORL_TASK_POINTGOAL; }
    else if (z < T(0.05)) { done = 1; }
    else if (P.task == SOLORL_TASK_POINTGOAL && E.goals > E.egoals) { E.egoals = E.goals; done = 1; su = 1; }
  }
  if (done && !nanr) {   // baseEnv.py:52-60
    if (su) { if (P.task == SOLORL_TASK_POINTGOAL) reward = T(0.1) * T(P.episode_length - E.timestep); }
    else if (!to) reward = T(-10);
  }
  out.rew[env] = (float)reward;
  out.done[env] = (unsigned char)done;
  if (out.timeout) out.timeout[env] = (unsigned char)to;
  if (out.success) out.success[env] = (unsigned char)su;
  if (out.nan_reset) out.nan_reset[env] = (unsigned char)nanr;
  if (out.ep_len) out.ep_len[env] = E.timestep;
  if (out.ep_rew) out.ep_rew[env] = (float)reward;
  if (out.goals) out.goals[env] = (float)E.egoals;
  if (out.dr0) out.dr0[env] = (float)E.dr[0];
  if (out.dr1) out.dr1[env] = (float)E.dr[1];
  if (out.dr2) out.dr2[env] = (float)E.dr[2];
  if (out.dr3) out.dr3[env] = (float)E.dr[3];
  if (out.dr4) out.dr4[env] = (float)E.dr[4];
  if (done && out.ep_stats) {      // finished-episode accumulators, one column per env (agents/ppo/train.py:90-100)
    float* s = out.ep_stats + env;
    const idx_t NN = (idx_t)N;
    if (nanr) s[9 * NN] += 1.0f;
    else {
      s[0] += 1.0f; s[NN] += (float)reward; s[2 * NN] += (float)E.timestep; s[3 * NN] += (float)su;
#pragma unroll
      for (int k = 0; k < 5; k++) s[(4 + k) * NN] += (float)E.dr[k];
    }
  }
  return done;
}
// The draws of the auto-reset (agents/ppo/envs.py:39 -> baseEnv.py:70-82) from the env's own Philox counter, in the reference's order:
// treadmill side (scene.reset inside robot.reset, solo.py:166-168), goal (robot.reset), settle count (env.reset).  Returns the snapshot slot.
template <typename T, int NQ>
SD int reset_draws(Env<T, NQ>& E, const EnvParams& P, long long gid) {
  int side = 0;
  if (P.use_treadmill) {
    unsigned rt[4];
    philox(P.seed_lo, P.seed_hi, (unsigned)gid, (unsigned)((unsigned long long)gid >> 32), (unsigned)E.rng++, 3u, rt);
    side = (rt[0] & 1u) ? 0 : 1;               // 0: strip centred on +offset, 1: on -offset (second half of the snapshot table)
  }
  if (P.task == SOLORL_TASK_POINTGOAL) sample_goal(E, P, gid);
  unsigned r[4];
  philox(P.seed_lo, P.seed_hi, (unsigned)gid, (unsigned)((unsigned long long)gid >> 32), (unsigned)E.rng++, 2u, r);
  return (int)(r[0] % (unsigned)P.nsettle) + side * P.nsettle;
}

// SoloBaseEnv.reset (baseEnv.py:70-82) in O(1): load the pre-simulated post-settle state of the slot reset_draws picks.
template <typename T, int ROBOT>
SD void reset_from_snapshot(Env<T, Robot<ROBOT>::NQ>& E, T* sf, const Layout& L, idx_t N, idx_t e, idx_t env, const T* snf,
                            const int* sni, int M, const EnvParams& P) {
  constexpr int NQ = Robot<ROBOT>::NQ;
  const int k = reset_draws(E, P, P.id0 + (long long)env);
  const int rng = E.rng;
  const T g0 = E.goal[0], g1 = E.goal[1];
  Env<T, NQ> S;
  load_env(S, snf, sni, L, (idx_t)M, (idx_t)k);
  E = S;
  E.rng = rng; E.timestep = 0;
  E.goal[0] = g0; E.goal[1] = g1; E.goals = T(0); E.egoals = T(0);
#pragma unroll
  for (int q = 0; q < 5; q++) E.dr[q] = T(0);
  for (int p = 0; p < NPRIM; p++) sf[SX(L.lam + p, e, L.NF)] = snf[SX(L.lam + p, k, L.NF)];
  for (int h = 0; h < L.H; h++)
    for (int d = 0; d < L.D; d++) sf[SX(L.hist + h * HSTRIDE + d, e, L.NF)] = snf[SX(L.hist + h * HSTRIDE + d, k, L.NF)];
  if (P.task == SOLORL_TASK_POINTGOAL) {
    for (int h = 0; h < L.H; h++) {
      sf[SX(L.hist + h * HSTRIDE + L.D - 2, e, L.NF)] = g0 * T(0.5);
      sf[SX(L.hist + h * HSTRIDE + L.D - 1, e, L.NF)] = g1 * T(0.5);
    }
    T dx = E.ps.pos.x - g0, dy = E.ps.pos.y - g1, px = E.xyprev[0] - g0, py = E.xyprev[1] - g1;
    E.pot = sqrt(dx * dx + dy * dy);
    E.prog = -(E.pot - sqrt(px * px + py * py));
  }
}

template <typename T, int ROBOT>
SD void write_obs(const Env<T, Robot<ROBOT>::NQ>& E, const T* sf, const Layout& L, idx_t N, idx_t e, idx_t env, int task, float* obs) {
  T cs[DMAX];
  current_state<T, ROBOT>(E, task, cs);
  const int O = L.D * (1 + L.H);
  float* o = obs + env * (idx_t)O;
  // SoloBase.calc_state, solo.py:186-196: [s, s - hist_newest, s - hist_older].  All history loads are issued
  // before the first store: obs and the state may alias as far as the compiler knows, and a load -> wait ->
  // store chain per element cost 38 dependent memory round trips (13 us of a 210 us step).
  T hv[2][DMAX];
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int d = 0; d < DMAX; d++) hv[h][d] = (h < L.H && d < L.D) ? sf[SX(L.hist + h * HSTRIDE + d, e, L.NF)] : T(0);
#pragma unroll
  for (int d = 0; d < DMAX; d++)
    if (d < L.D) {
      o[d] = (float)cs[d];
#pragma unroll
      for (int h = 0; h < 2; h++)
        if (h < L.H) o[(h + 1) * L.D + d] = (float)(cs[d] - hv[h][d]);
      for (int h = 2; h < L.H; h++) o[(h + 1) * L.D + d] = (float)(cs[d] - sf[SX(L.hist + h * HSTRIDE + d, e, L.NF)]);    // (deeper levels: straight from HBM)
    }
}

// ---------------------------------------------------------------- lane mode (SOLORL_TEAM=0): one env per lane
// 64 envs per wavefront, the env in registers, rows in LDS.  Kept as an independent second implementation of the step's
// physics and data movement (substep vs substep_team; GPU test: lane vs team vs sorted storage agree); the scalar env logic
// above is shared with step_team below, the default, and has the oracle as its independent reference.
template <typename T, int ROBOT>
SD void step_body(T* __restrict__ sf, int* __restrict__ si, const T* __restrict__ snf, const int* __restrict__ sni, int M,
                  const Layout& L, int N, const EnvParams& P, const PhysParams<T>& pp, const float* __restrict__ actions,
                  const Outputs& out, int mode) {
  using RB = Robot<ROBOT>;
  constexpr int NQ = RB::NQ;
  using LDS = RowLds<T>;
  constexpr int EPB = LDS::LANES;          // envs per workgroup: compile-time (LDS immediates)
  const int col = threadIdx.x;
  idx_t e = (idx_t)blockIdx.x * EPB + col;
  if (e >= (idx_t)N) return;
  LDS lds; lds.lanes = EPB; lds.lane = col;
  Env<T, NQ> E;
  const idx_t env = (idx_t)si[SX(I_ENVID, e, NI)];   // state is kept sorted by contact count: slot e holds env `env`
  load_env(E, sf, si, L, (idx_t)N, e);

  // ---- A3 apply_action
  T tau[NQ], asq = T(0);
#pragma unroll
  for (int j = 0; j < NQ; j++) {
    T a = mode == MODE_STEP ? (T)actions[env * NQ + j] : T(0);
    asq += a * a;
    T c = a < T(-1) ? T(-1) : (a > T(1) ? T(1) : a);
    if (P.control == SOLORL_CONTROL_TORQUE) tau[j] = c * T(P.max_torque);
    else {
      T t = T(P.kp) * (c * pp.qlim - E.ps.q[j]) - T(P.kd) * E.ps.qd[j];
      tau[j] = clampv(t, T(P.max_torque));
    }
    if (mode != MODE_STEP) tau[j] = T(0);
    if (out.tau && mode == MODE_STEP) out.tau[env * NQ + j] = (float)tau[j];
  }

  // ---- A4 simulator_step: history push (pre-step state), frame_skip sub-steps
  if (L.H > 0) {
    T cs[DMAX], h0[DMAX];
    current_state<T, ROBOT>(E, P.task, cs);
    for (int lv = L.H - 1; lv >= 2; lv--)              // levels beyond the second (num_history_stack 3, 4) shift in HBM, oldest first
      for (int d = 0; d < L.D; d++) sf[SX(L.hist + lv * HSTRIDE + d, e, L.NF)] = sf[SX(L.hist + (lv - 1) * HSTRIDE + d, e, L.NF)];
#pragma unroll
    for (int d = 0; d < DMAX; d++) h0[d] = (L.H >= 2 && d < L.D) ? sf[SX(L.hist + d, e, L.NF)] : T(0);   // loads first (see write_obs)
#pragma unroll
    for (int d = 0; d < DMAX; d++)
      if (d < L.D) {
        if (L.H >= 2) sf[SX(L.hist + HSTRIDE + d, e, L.NF)] = h0[d];
        sf[SX(L.hist + d, e, L.NF)] = cs[d];
      }
  }
  E.xyprev[0] = E.ps.pos.x; E.xyprev[1] = E.ps.pos.y;
  {
    SubCtx<T, ROBOT> C;
    C.ps = E.ps; C.tmy = E.tmy;
#pragma unroll 1
    for (int ss = 0; ss < P.frame_skip; ss++) {
      const T sc = (ss == 0 || P.hold_torque) ? T(1) : T(0);   // K8: Bullet clears applied torques every step
#pragma unroll
      for (int j = 0; j < NQ; j++) C.tau[j] = tau[j] * sc;
      E.mask = substep<T, ROBOT>(C, pp, sf + SX(L.lam, e, L.NF), 4u, lds);
    }
    E.ps = C.ps;
  }
  if (P.task == SOLORL_TASK_POINTGOAL && mode == MODE_STEP) pointgoal_progress(E, P, P.id0 + (long long)env);
  if (mode == MODE_SETTLE) { store_env(E, sf, si, L, (idx_t)N, e); return; }
  E.timestep += 1;
  const int done = reward_termination_outputs<T, NQ>(E, P, asq, out, env, N);     // A7, A8, A1, outputs

  // ---- auto-reset (agents/ppo/envs.py:39) and observation
  if (done) reset_from_snapshot<T, ROBOT>(E, sf, L, (idx_t)N, e, env, snf, sni, M, P);
  write_obs<T, ROBOT>(E, sf, L, (idx_t)N, e, env, P.task, out.obs);
  store_env(E, sf, si, L, (idx_t)N, e);
}

#ifdef SOLO_WAVE_TIMING
#define WT_STAMP(i) do { wts_[i] = clock64(); } while (0)
#else
#define WT_STAMP(i) do {} while (0)
#endif

// ---------------------------------------------------------------- team mode (default): the whole step on 16 lanes per env
// sum over the 16 lanes of a team (every lane ends with the total)
template <typename T> SD T team_sum16(T x) {
  if constexpr (sizeof(T) == 4) {
    x += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    x += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    x += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x141, 0xF, 0xF, true));   // row_half_mirror
    x += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x140, 0xF, 0xF, true));   // row_mirror
  } else {
    x += __shfl_xor(x, 1, 16); x += __shfl_xor(x, 2, 16); x += __shfl_xor(x, 4, 16); x += __shfl_xor(x, 8, 16);
  }
  return x;
}
enum { ER_GOAL = 0, ER_POT = 2, ER_PROG = 3, ER_GOALS = 4, ER_EGOALS = 5, ER_DR = 6, ER_XYPREV = 11, ER_TMY = 13, NER = 14 };   // SubCtx::erec
enum { IR_TIMESTEP = 0, IR_MASK = 1, IR_RNG = 2, IR_SNAP = 3, IR_DONE = 4 };                                                  // SubCtx::irec
template <typename T, int ROBOT> SD void env_from_lds(Env<T, Robot<ROBOT>::NQ>& E, const SubCtx<T, ROBOT>& C) {
  E.ps = C.ps;
  E.goal[0] = C.erec[ER_GOAL]; E.goal[1] = C.erec[ER_GOAL + 1]; E.pot = C.erec[ER_POT]; E.prog = C.erec[ER_PROG];
  E.goals = C.erec[ER_GOALS]; E.egoals = C.erec[ER_EGOALS];
#pragma unroll
  for (int k = 0; k < 5; k++) E.dr[k] = C.erec[ER_DR + k];
  E.xyprev[0] = C.erec[ER_XYPREV]; E.xyprev[1] = C.erec[ER_XYPREV + 1]; E.tmy = C.erec[ER_TMY];
  E.timestep = C.irec[IR_TIMESTEP]; E.mask = C.irec[IR_MASK]; E.rng = C.irec[IR_RNG];
}
template <typename T, int ROBOT> SD void scalars_to_lds(const Env<T, Robot<ROBOT>::NQ>& E, SubCtx<T, ROBOT>& C) {
  C.erec[ER_GOAL] = E.goal[0]; C.erec[ER_GOAL + 1] = E.goal[1]; C.erec[ER_POT] = E.pot; C.erec[ER_PROG] = E.prog;
  C.erec[ER_GOALS] = E.goals; C.erec[ER_EGOALS] = E.egoals;
#pragma unroll
  for (int k = 0; k < 5; k++) C.erec[ER_DR + k] = E.dr[k];
  C.erec[ER_XYPREV] = E.xyprev[0]; C.erec[ER_XYPREV + 1] = E.xyprev[1]; C.erec[ER_TMY] = E.tmy;
  C.irec[IR_TIMESTEP] = E.timestep; C.irec[IR_MASK] = E.mask; C.irec[IR_RNG] = E.rng;
}

// current_state (above) spread over the team: lane t produces elements t, t + 16, t + 32 straight from the LDS context -- one read and
// one multiply each; the three euler angles on lanes 1..3, every one of them running the leader's euler_zyx (same instructions, same
// bits) and keeping its own angle.  Replaces: the leader copying the whole context to registers (54 reads), computing the D values,
// staging them through LDS (D stores, a team sync, a read per lane).  Element map: current_state.
template <typename T, int ROBOT, int HK_>
SD void team_current_state(const SubCtx<T, ROBOT>& C, int task, int D, int t, T (&cs)[HK_]) {
  constexpr int NQ = Robot<ROBOT>::NQ;
  using PS_ = PhysState<T, NQ>;
  static_assert(offsetof(PS_, v) == 7 * sizeof(T) && offsetof(PS_, q) == 13 * sizeof(T) && sizeof(PS_) == (13 + 2 * NQ) * sizeof(T),
                "PhysState is a flat array: pos 0-2, quat 3-6, v 7-9, w 10-12, q, qd");
  const T* psv = reinterpret_cast<const T*>(&C.ps);
  const int mask = C.irec[IR_MASK];
  const T g0 = C.erec[ER_GOAL], g1 = C.erec[ER_GOAL + 1];
  T ang = T(0);
  if (t >= 1 && t <= 3) {
    T r, p, y;
    euler_zyx(C.ps.qx, C.ps.qy, C.ps.qz, C.ps.qw, r, p, y);
    const T a = t == 1 ? r : (t == 2 ? p : y);
    ang = (a - T(2) * floor(a * T(0.5))) * T(0.5);   // (euler % 2*pi)/(2*pi) == (euler % 2)/2, solo.py:206
  }
#pragma unroll
  for (int k = 0; k < HK_; k++) {
    const int d = t + 16 * k;
    const int e = d - (14 + 2 * NQ);                       // pointgoal extras: pos.x, pos.y, goal x, goal y (all * 0.5)
    const int idx = d == 0 ? 2 : (d < 10 + 2 * NQ ? d + 3 : (e >= 0 && e < 2 ? e : 0));
    const T raw = psv[idx];
    const T sc = d < 10 ? T(1) : (d < 10 + NQ ? T(0.1) : (d < 10 + 2 * NQ ? T(0.01) : T(0.5)));     // (/10, /100: solo.py:208-209)
    T v = raw * sc;
    if (d >= 1 && d <= 3) v = ang;
    const int f = d - (10 + 2 * NQ);
    if (f >= 0 && f < 4) v = ((mask >> (13 + 2 * f)) & 1) ? T(1) : T(0);     // solo.py:310-323 (see current_state)
    if (e == 2) v = g0 * T(0.5);
    if (e == 3) v = g1 * T(0.5);
    if (task != SOLORL_TASK_POINTGOAL && e >= 0) v = T(0);
    cs[k] = d < D ? v : T(0);
  }
}

// One launch = SoloBaseEnv.step for every env, 16 lanes (one DPP row) per env, 4 envs per wavefront.  Everything on the
// wavefront's critical path is spread over the team's lanes: the env's state travels HBM <-> LDS with all 16 lanes (4 loads
// per lane instead of 61 on one), joint t's action, clip and PD torque are lane t's, history / observation / impulse cache /
// snapshot reset are moved by all lanes; only the scalar env logic (euler angles, reward, termination, Philox draws) runs on
// the team leader, on values it reads from LDS.  Nothing but the six history values a lane needs for the observation deltas
// stays in registers across the sub-steps (the round-1 version kept the env there: 56 spilled VGPRs per wavefront and step,
// 11 MB of scratch write-back per launch against 5.7 MB of algorithmic traffic).
// ---------------------------------------------------------------- Policy.act in the step kernel's tail (solorl_step_act)
// agents/ppo/policy.py:33-49 on the MLP of :62-81 (two tanh MLPs obs -> 64 -> 64, critic head -> 1, actor head -> A, state-independent
// log-std) for the env whose observation this team has just produced.  Why here: at 4096 envs the launch lasts as long as its slowest
// wavefront while the MEAN wavefront is done after half that time, and the rollout's next launch -- the policy --
// can only start when the launch has drained; computed by each wavefront for its own four envs the policy rides in that idle time and
// a rollout step is ONE launch.  Hidden layers: one unit per lane for the wavefront's four envs (pol_layer); activations are exchanged
// through the (now dead) row storage in LDS, weights come from L2 as float4 rows (PyTorch layout); heads: 16 lanes per env, lanes 0..A-1
// the actor head, lane 15 the critic head.  ~1500 instructions per wavefront (~3 us) against a 15 us kernel + launch gap.  O % 4 == 0
// (one history level).
constexpr float POL_HALF_LOG_2PI = 0.91893853320467274178f;
constexpr unsigned POL_ENV_BYTES = 2496;     // per-env slice of the row storage (26 rows x 24 values x 4 B): obs <= 96, h1 128, h2 128 floats
static_assert(POL_ENV_BYTES == MAX_ROWS * (ROW_CORE + 4) * sizeof(float), "the policy tail's per-env slice is one env's fp32 row storage (RowLds)");
static_assert((224 + 128) * sizeof(float) <= POL_ENV_BYTES, "the last activation block (h2: 128 floats at float offset 224) must end inside the slice");
SD float pol_tanh(float x) { const float e = __expf(2.0f * x); return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + e); }   // as solorl_ppo.hip tanh_fast
typedef float nfloat4 __attribute__((ext_vector_type(4)));          // (native vector: HIP's float4 class cannot be read through an address-space pointer)
typedef __attribute__((address_space(1))) const nfloat4 gfloat4;
SD float pol_dot4(nfloat4 w, nfloat4 x, float acc) { return fmaf(w.x, x.x, fmaf(w.y, x.y, fmaf(w.z, x.z, fmaf(w.w, x.w, acc)))); }
// A lone wavefront has nothing to hide a load's latency behind, so the weight loads are issued in explicit BATCHES (16-20 float4 per
// batch) with a compiler barrier behind them that also re-defines the loaded values -- left to itself the scheduler kept ~8 loads in
// flight and waited for them one or two at a time (19 exposed L2 round trips in layer 1 alone: the tail took 29 us).
#define POL_PIN4(x) asm volatile("" : "+v"(x))
// Hidden layers, one UNIT per lane: lane L of the wavefront computes unit L of both nets for all FOUR envs of the wavefront -- a weight row
// is loaded once per wavefront and multiplied with four observation vectors (LDS broadcast reads) instead of once per env: 70 float4
// weight loads per lane for the two layers instead of 280.
// One batch of weights: KB input chunks (float4) of lane L's row of both nets, issued together; and its multiply-adds against the four envs'
// inputs.  policy_tail_team strings five batches into a software pipeline: the NEXT batch's loads are issued before the current batch's
// arithmetic, so only the first round trip is exposed.
template <int KB> struct PolBatch { nfloat4 c[KB], a[KB]; };
template <int KB>
SD void pol_load(PolBatch<KB>& B, const float* wc_, const float* wa_, int K4, int k0, int lane) {
  gfloat4* wc = (gfloat4*)(wc_ + (size_t)lane * 4 * K4);
  gfloat4* wa = (gfloat4*)(wa_ + (size_t)lane * 4 * K4);
#pragma unroll
  for (int kk = 0; kk < KB; kk++) {
    const int k = k0 + kk < K4 ? k0 + kk : K4 - 1;          // (past the end: the last chunk again, not accumulated)
    B.c[kk] = wc[k]; B.a[kk] = wa[k];
  }
  asm volatile("" ::: "memory");                            // issued HERE (the scheduler would otherwise move them to their uses)
}
template <int KB>
SD void pol_fma(PolBatch<KB>& B, int K4, int k0, unsigned xoff, unsigned xoff_a, float (&c)[4], float (&a)[4]) {
  asm volatile("" ::: "memory");
#pragma unroll
  for (int kk = 0; kk < KB; kk++) { POL_PIN4(B.c[kk]); POL_PIN4(B.a[kk]); }
#pragma unroll
  for (int kk = 0; kk < KB; kk++)
    if (k0 + kk < K4) {
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const nfloat4 xc = reinterpret_cast<const nfloat4*>(solo_smem + e * POL_ENV_BYTES + xoff)[k0 + kk];
        const nfloat4 xa = xoff_a == xoff ? xc : reinterpret_cast<const nfloat4*>(solo_smem + e * POL_ENV_BYTES + xoff_a)[k0 + kk];
        c[e] = pol_dot4(B.c[kk], xc, c[e]); a[e] = pol_dot4(B.a[kk], xa, a[e]);
      }
    }
}
SD void pol_act_store(const float (&c)[4], const float (&a)[4], unsigned yoff, int lane) {
#pragma unroll
  for (int e = 0; e < 4; e++) {
    float* y = reinterpret_cast<float*>(solo_smem + e * POL_ENV_BYTES + yoff);
    y[lane] = pol_tanh(c[e]); y[64 + lane] = pol_tanh(a[e]);
  }
}

template <int A>
SD void policy_tail_team(const PolicyTail& P, int O, int col, int t, idx_t env, bool valid) {
  float* const buf = reinterpret_cast<float*>(solo_smem + (unsigned)col * POL_ENV_BYTES);
  float* const h2 = buf + 224;              // per env: obs at 0 (<= 96 floats), h1 at 96 [critic 64 | actor 64], h2 at 224
  const int lane = threadIdx.x & 63, O4 = O >> 2;
  static_assert(A < 15, "the critic head sits on lane 15");
  const bool head = t < A || t == 15;
  constexpr unsigned H1 = 96u * 4u, H2 = 224u * 4u;
  float c[4], a[4];
  // layer 1 (both nets read the observation) in two batches, layer 2 (critic reads h1[0..63], actor h1[64..127]) in two, then the heads' rows
  PolBatch<11> w1a, w1b;                    // (two batches of 11 chunks: observations of up to 88 values; the widest is 84)
  PolBatch<8> w2a, w2b;
  nfloat4 whb[16];
  pol_load(w1a, P.cw0, P.aw0, O4, 0, lane);
  pol_load(w1b, P.cw0, P.aw0, O4, 11, lane);
#pragma unroll
  for (int e = 0; e < 4; e++) { c[e] = P.cb0[lane]; a[e] = P.ab0[lane]; }
  pol_fma(w1a, O4, 0, 0u, 0u, c, a);
  pol_load(w2a, P.cw1, P.aw1, 16, 0, lane);
  pol_fma(w1b, O4, 11, 0u, 0u, c, a);
  pol_act_store(c, a, H1, lane);
  pol_load(w2b, P.cw1, P.aw1, 16, 8, lane);
#pragma unroll
  for (int e = 0; e < 4; e++) { c[e] = P.cb1[lane]; a[e] = P.ab1[lane]; }
  TEAM_SYNC();
  pol_fma(w2a, 16, 0, H1, H1 + 256u, c, a);
  {
    gfloat4* wh = (gfloat4*)(t == 15 ? P.cw2 : P.mw + (size_t)(head ? t : 0) * 64);
#pragma unroll
    for (int k = 0; k < 16; k++) whb[k] = wh[k];
    asm volatile("" ::: "memory");
  }
  pol_fma(w2b, 16, 8, H1, H1 + 256u, c, a);
  pol_act_store(c, a, H2, lane);
  TEAM_SYNC();
  // heads: lane t < A -> mean_t (and the action, its log-prob term), lane 15 -> value
  float out = 0.f;
  {
    asm volatile("" ::: "memory");
#pragma unroll
    for (int k = 0; k < 16; k++) POL_PIN4(whb[k]);
    const nfloat4* x = reinterpret_cast<const nfloat4*>(t == 15 ? h2 : h2 + 64);
    float o0 = t == 15 ? P.cb2[0] : P.mb[head ? t : 0], o1 = 0.f;        // (two chains: the head is 64 dependent multiply-adds otherwise)
#pragma unroll
    for (int k = 0; k < 16; k += 2) { o0 = pol_dot4(whb[k], x[k], o0); o1 = pol_dot4(whb[k + 1], x[k + 1], o1); }
    out = head ? o0 + o1 : 0.f;
  }
  float lp = 0.f, act = out;
  if (t < A) {
    const float ls = P.logstd[t];
    const float nz = P.noise ? P.noise[(size_t)env * A + t] : 0.f;
    act = out + __expf(ls) * nz;                                   // policy.py:41-45: mean + std * noise (noise null: the mean)
    lp = -0.5f * nz * nz - ls - POL_HALF_LOG_2PI;                  // log N(action; mean, std) = sum over dims, z = noise
  }
  lp = team_sum16(lp);
  if (valid) {
    if (t < A) P.action[(size_t)env * A + t] = act;
    if (t == 15) P.value[env] = out;
    if (t == 0) P.logp[env] = lp;
  }
}

// DUO (duo_kernel_team): the workgroup has a second wavefront, the HELPER, which runs the collision front of every sub-step while
// this one, the main wavefront, computes the leg dynamics, then the leg sum, the base solve and the leg rates while this one parks
// the leg rows, and the base's pose integration (with the next sub-step's R0) while this one integrates the joints
// (substep_team_helper); both address the workgroup's one LDS block with the lane index threadIdx.x & 63.  The helper loads nothing
// from HBM and stores nothing to it.
template <typename T, int ROBOT, bool DUO = false>
SD void step_team(T* __restrict__ sf, int* __restrict__ si, const T* __restrict__ snf, const int* __restrict__ sni, int M,
                  const Layout& L, int N, const EnvParams& P, const PhysParams<T>& pp, const float* __restrict__ actions,
                  const Outputs& out, int mode) {
  using RB = Robot<ROBOT>;
  constexpr int NQ = RB::NQ, NPS = 13 + 2 * NQ;
  using LDS = RowLds<T, 4>;
  using CH = typename TeamCtx<T, ROBOT, LDS>::type;
  static_assert(sizeof(PhysState<T, NQ>) == NPS * sizeof(T), "PhysState is the HBM field order pos, quat, v, w, q, qd");
#ifdef SOLO_WAVE_TIMING
  long long wts_[11];
  for (int i_ = 0; i_ < 11; i_++) wts_[i_] = 0;
  const long long wr0_ = wall_clock64();
  if (threadIdx.x < 16) solo::solo_pt_acc[threadIdx.x] = 0;
  __syncthreads();
  wts_[0] = clock64();
#endif
  const unsigned wlane = DUO ? (threadIdx.x & 63u) : threadIdx.x;      // lane of the wavefront (DUO: two wavefronts share the block)
  const int t = wlane & 15, col = wlane >> 4;
  // a workgroup touches only 16 B of each state field, so eight consecutive workgroups share every 128-B line; workgroup
  // ids go round-robin over the 8 XCDs (each with its own L2), hence give every XCD one CONTIGUOUS eighth of the env range
  // instead of every eighth workgroup (grid is a multiple of 8).
  const unsigned blk = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  idx_t e = (idx_t)blk * 4 + col;
  const bool valid = e < (idx_t)N;
  if (!valid) e = (idx_t)N - 1;           // every lane stays alive for the wave-level exchanges
  const bool lead = valid && t == 0;
  LDS lds; lds.lanes = 4; lds.lane = col;
  // test hook (SOLORL_POISON_LDS=<word>, read at create): pre-fill the whole dynamic LDS.  Two runs with different fill words
  // (NaN vs 0) must agree bitwise -- anything read before it is written in the launch breaks that
  // (tests/test_parity_gpu.py::test_no_lds_read_before_write; this is how a lane hand-off race was found)
  if (P.lds_poison_on) {
    using TC = TeamCtx<T, ROBOT, LDS>;
    unsigned* w = reinterpret_cast<unsigned*>(solo_smem);
    for (unsigned k = wlane; k < TC::bytes / 4; k += 64) w[k] = P.lds_poison;     // (DUO: both wavefronts, the same words)
    __syncthreads();
  }
  const CH ch{col};
  SubCtx<T, ROBOT>& C = ch.get();
  T* const psv = reinterpret_cast<T*>(&C.ps);
  if constexpr (DUO) {
    // Workgroup barriers of a step, per role: 5 x frame_skip + 1 (A, B, C, C2 and D of every sub-step, then Z; main: A in substep_team, B in
    // phase_leg_rt, C, C2 and D in duo_join_rows, Z in duo_join_rows below the sub-step loop; helper: A and B in substep_team_helper, C in
    // duo_helper_rates, C2 and D in duo_join_rows, Z in duo_join_rows below its loop) -- plus the one behind the LDS poison fill above when
    // that test hook is on, and, in a -DSOLO_WAVE_TIMING build, the one behind the counters' reset.  All of them sit on paths that
    // depend on kernel arguments only; the helper returns behind Z.
    if (blk * 4u >= (unsigned)N) return;              // a workgroup of the padded grid without an env: both wavefronts leave here
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) {          // ---- the helper wavefront
#pragma unroll 1
      for (int ss = 0; ss < P.frame_skip; ss++)
        substep_team_helper<T, ROBOT>(pp, lds, t, lead, valid, ss + 1 < P.frame_skip);
      duo_join_rows<T, ROBOT>();                      // barrier Z: the last sub-step's base pose is in LDS
      return;
    }
    // an idle team of a workgroup that has envs runs the leg phase with the others (barrier B is inside): it parks nothing
    if (!valid && t == 0) { C.mask = 0; C.nc = 0; C.nlim_total = 0; C.lsel = 0; C.smask = 0; }
  }
  idx_t env = 0;
  // ---- the env's state, HBM -> LDS, all lanes (the state is stored by slot: slot e holds env `env`)
  T a_t = T(0);
  if (valid) {
    env = P.linear_ids ? e : (idx_t)si[SX(I_ENVID, e, NI)];      // (the action load below depends on it: one HBM round trip less)
    for (int f = t; f < NPS; f += 16) psv[f] = sf[SX(L.pos + f, e, L.NF)];
    if (t < NER) C.erec[t] = sf[SX(L.goal + t, e, L.NF)];
    if (t < 3) C.irec[t] = si[SX(t, e, NI)];
    for (int p = t; p < NPRIM; p += 16) C.lamp[p] = sf[SX(L.lam + p, e, L.NF)];
    if (t < NQ && mode == MODE_STEP) a_t = (T)actions[env * NQ + t];
  }
  static_assert(I_TIMESTEP == IR_TIMESTEP && I_MASK == IR_MASK && I_RNG == IR_RNG, "counter order");
  TEAM_SYNC();
  WT_STAMP(1);
  // ---- A3 apply_action (solo.py:224-259, controllers/PD.py:3-10): joint t on lane t
  if (valid && t < NQ) {
    const T c = a_t < T(-1) ? T(-1) : (a_t > T(1) ? T(1) : a_t);
    T tq;
    if (P.control == SOLORL_CONTROL_TORQUE) tq = c * T(P.max_torque);
    else tq = clampv(T(P.kp) * (c * pp.qlim - C.ps.q[t]) - T(P.kd) * C.ps.qd[t], T(P.max_torque));
    C.tau_base[t] = mode == MODE_STEP ? tq : T(0);
    if (out.tau && mode == MODE_STEP) out.tau[env * NQ + t] = (float)tq;
  }
  const T asq = team_sum16(a_t * a_t);        // sum of the raw, unclipped action squares (baseEnv.py:142-144)
  WT_STAMP(2);
  // ---- A4 simulator_step: history push (pre-step state).  The leader publishes the D state values through LDS (the `bc`
  // block is free outside the sub-steps) and lane t moves elements t, t+16, t+32 -- 64-B coalesced segments -- keeping what
  // it wrote (hk0 = new newest = pre-step state, hk1 = old newest) for the observation at the end.
  constexpr int HK = (DMAX + 15) / 16;
  T hk0[HK], hk1[HK];
#pragma unroll
  for (int k = 0; k < HK; k++) { hk0[k] = T(0); hk1[k] = T(0); }
  T csk[HK];
  if (L.H > 0) team_current_state<T, ROBOT, HK>(C, P.task, L.D, t, csk);
  TEAM_SYNC();                 // (the leader's stores below: behind every lane's reads of the pre-step context)
  if (lead) {
    C.erec[ER_XYPREV] = C.ps.pos.x; C.erec[ER_XYPREV + 1] = C.ps.pos.y;
    C.tmy = C.erec[ER_TMY];
    // DUO: the first sub-step's R0 is this wavefront's; every later one is the helper's, left behind the previous sub-step's barrier D
    if constexpr (DUO) C.R0 = quat_to_mat(C.ps.qx, C.ps.qy, C.ps.qz, C.ps.qw);
  }
  if (valid && L.H > 0) {
#pragma unroll
    for (int k = 0; k < HK; k++) {
      const int d = t + 16 * k;
      if (d < L.D) {
        const T c = csk[k];
        for (int lv = L.H - 1; lv >= 2; lv--)          // levels beyond the second (num_history_stack 3, 4) shift in HBM, oldest first; same lane, same elements
          sf[SX(L.hist + lv * HSTRIDE + d, e, L.NF)] = sf[SX(L.hist + (lv - 1) * HSTRIDE + d, e, L.NF)];
        if (L.H >= 2) { hk1[k] = sf[SX(L.hist + d, e, L.NF)]; sf[SX(L.hist + HSTRIDE + d, e, L.NF)] = hk1[k]; }
        sf[SX(L.hist + d, e, L.NF)] = c;
        hk0[k] = c;
      } else if (d < ((L.D + 3) & ~3)) {               // (pad: the level's last sector is written whole)
        sf[SX(L.hist + d, e, L.NF)] = T(0);
        for (int lv = 1; lv < L.H; lv++) sf[SX(L.hist + lv * HSTRIDE + d, e, L.NF)] = T(0);
      }
    }
  }
  WT_STAMP(3);
  // ---- frame_skip physics sub-steps
#pragma unroll 1
  for (int ss = 0; ss < P.frame_skip; ss++) {
    const T sc = (ss == 0 || P.hold_torque) ? T(1) : T(0);   // K8: Bullet clears applied torques every step
    if (valid && t < NQ) C.tau[t] = C.tau_base[t] * sc;
    const int m = substep_team<T, ROBOT, LDS, DUO>(pp, sf + SX(L.lam, e, L.NF), 4u, lds, t, lead, valid);
    if (lead) C.irec[IR_MASK] = m;
  }
  if constexpr (DUO) {
    duo_join_rows<T, ROBOT>();           // barrier Z: the helper's last base pose is in LDS (it returns behind this barrier)
  }
  WT_STAMP(4);
  if (valid) for (int p = t; p < NPRIM; p += 16) sf[SX(L.lam + p, e, L.NF)] = C.lamp[p];
  WT_STAMP(5);
  // ---- scalar env logic on the leader (values from LDS)
  if (lead) {
    Env<T, NQ> E;
    env_from_lds<T, ROBOT>(E, C);
    int done = 0;
    if (P.task == SOLORL_TASK_POINTGOAL && mode == MODE_STEP) pointgoal_progress(E, P, P.id0 + (long long)env);
    if (mode == MODE_STEP) {
      E.timestep += 1;
      done = reward_termination_outputs<T, NQ>(E, P, asq, out, env, N);     // A7, A8, A1, outputs
      if (done) C.irec[IR_SNAP] = reset_draws(E, P, P.id0 + (long long)env);     // auto-reset, part 1: the draws
    }
    scalars_to_lds<T, ROBOT>(E, C);          // (a reset keeps the goal and the rng counter from here)
    C.irec[IR_DONE] = done;
  }
  WT_STAMP(6);
  TEAM_SYNC();
  const int done = valid ? C.irec[IR_DONE] : 0;
  if (done) {
    // ---- auto-reset, part 2 = SoloBaseEnv.reset in O(1): the pre-simulated post-settle state (snapshot slot) replaces the env's
    // state, every field moved by the team -- HBM for all of them, LDS too for what the rest of this step reads
    const idx_t k = (idx_t)C.irec[IR_SNAP], MM = (idx_t)M;
    for (int f = t; f < L.NF; f += 16) {
      const T v = snf[SX(f, k, L.NF)];
      const bool scalar = f >= L.goal && f < L.goal + NER;
      if (!scalar) sf[SX(f, e, L.NF)] = v;                     // (the scalars are stored at the end, patched)
      if (f < NPS) psv[f] = v;
      else if (scalar && f != L.goal && f != L.goal + 1) C.erec[f - L.goal] = v;     // (the goal just drawn stays)
    }
    if (t == 1) C.irec[IR_MASK] = sni[SX(I_MASK, k, NI)];
#pragma unroll
    for (int kk = 0; kk < HK; kk++) {          // this lane's history elements, for the observation deltas
      const int d = t + 16 * kk;
      if (d < L.D) {
        if (L.H >= 1) hk0[kk] = snf[SX(L.hist + d, k, L.NF)];
        if (L.H >= 2) hk1[kk] = snf[SX(L.hist + HSTRIDE + d, k, L.NF)];
      }
    }
    TEAM_SYNC();
    const T g0 = C.erec[ER_GOAL], g1 = C.erec[ER_GOAL + 1];
    if (P.task == SOLORL_TASK_POINTGOAL) {     // the history keeps the NEW goal (set before the settle steps, solo.py:170-176)
#pragma unroll
      for (int kk = 0; kk < HK; kk++) {
        const int d = t + 16 * kk;
        if (d == L.D - 2 || d == L.D - 1) {
          const T gv = (d == L.D - 2 ? g0 : g1) * T(0.5);
          if (L.H >= 1) { hk0[kk] = gv; sf[SX(L.hist + d, e, L.NF)] = gv; }
          if (L.H >= 2) { hk1[kk] = gv; sf[SX(L.hist + HSTRIDE + d, e, L.NF)] = gv; }
          for (int lv = 2; lv < L.H; lv++) sf[SX(L.hist + lv * HSTRIDE + d, e, L.NF)] = gv;
        }
      }
    }
    if (t == 0) {
      C.irec[IR_TIMESTEP] = 0;
      C.erec[ER_GOALS] = T(0); C.erec[ER_EGOALS] = T(0);
#pragma unroll
      for (int q = 0; q < 5; q++) C.erec[ER_DR + q] = T(0);
      if (P.task == SOLORL_TASK_POINTGOAL) {
        const T dx = C.ps.pos.x - g0, dy = C.ps.pos.y - g1, px = C.erec[ER_XYPREV] - g0, py = C.erec[ER_XYPREV + 1] - g1;
        const T pot = sqrt(dx * dx + dy * dy);
        C.erec[ER_POT] = pot; C.erec[ER_PROG] = -(pot - sqrt(px * px + py * py));
      }
    }
  }
  WT_STAMP(7);
  // ---- A6 observation (solo.py:186-196): [s, s - hist_newest, s - hist_older], element d on lane d mod 16
  const bool want_obs = mode == MODE_STEP;
  TEAM_SYNC();                 // (a reset's state, written by all lanes above)
  T cso[HK];
  if (want_obs) team_current_state<T, ROBOT, HK>(C, P.task, L.D, t, cso);
  WT_STAMP(8);
  bool with_policy = false;
  if constexpr (sizeof(T) == 4) with_policy = want_obs && out.pol.value != nullptr;         // (uniform: a kernel argument)
  if (valid) {
    if (want_obs) {
      float* o = out.obs + env * (idx_t)(L.D * (1 + L.H));
      float* ol = reinterpret_cast<float*>(solo_smem + (unsigned)col * POL_ENV_BYTES);       // the policy tail's copy (row storage: dead by now)
#pragma unroll
      for (int k = 0; k < HK; k++) {
        const int d = t + 16 * k;
        if (d < L.D) {
          const T c = cso[k];
          o[d] = (float)c;
          if (L.H >= 1) o[L.D + d] = (float)(c - hk0[k]);
          if (L.H >= 2) o[2 * L.D + d] = (float)(c - hk1[k]);
          for (int lv = 2; lv < L.H; lv++) {
            // levels beyond the second live in HBM only.  An env that was just reset reads its snapshot (the team's copy above was
            // written by OTHER lanes) with the new goal patched in; any other env reads what this same lane shifted at the history push
            T hv;
            if (done) {
              hv = snf[SX(L.hist + lv * HSTRIDE + d, (idx_t)C.irec[IR_SNAP], L.NF)];
              if (P.task == SOLORL_TASK_POINTGOAL && d >= L.D - 2) hv = C.erec[ER_GOAL + (d - (L.D - 2))] * T(0.5);
            } else hv = sf[SX(L.hist + lv * HSTRIDE + d, e, L.NF)];
            o[(lv + 1) * L.D + d] = (float)(c - hv);
          }
          if (with_policy) {               // (only for obs sizes the policy kernels know: at most one history level)
            ol[d] = (float)c;
            if (L.H >= 1) ol[L.D + d] = (float)(c - hk0[k]);
          }
        }
      }
    }
    // ---- the env's state, LDS -> HBM, all lanes
    for (int f = t; f < ((NPS + 3) & ~3); f += 16) sf[SX(L.pos + f, e, L.NF)] = f < NPS ? psv[f] : T(0);     // (whole sectors:
    sf[SX(L.goal + t, e, L.NF)] = t < NER ? C.erec[t] : T(0);                                                 //  the pads are written too)
    if (t < 3) si[SX(t, e, NI)] = C.irec[t];
  }
  if constexpr (sizeof(T) == 4) {
    if (with_policy) {
      TEAM_SYNC();           // the observation copy, written by all lanes above
      policy_tail_team<NQ>(out.pol, L.D * (1 + L.H), col, t, env, valid);
    }
  }
  WT_STAMP(9);
#ifdef SOLO_WAVE_TIMING
  __builtin_amdgcn_s_waitcnt(0);     // (vmcnt = lgkmcnt = 0: the stores above have left)
  if (threadIdx.x == 0 && blockIdx.x < solo::SOLO_WT_WAVES) {
    wts_[10] = clock64();
    unsigned long long* w_ = solo::solo_wave_times[blockIdx.x];
    w_[0] = (unsigned long long)(wts_[3] - wts_[0]); w_[1] = (unsigned long long)(wts_[4] - wts_[3]); w_[2] = (unsigned long long)(wts_[10] - wts_[4]);
    w_[3] = (unsigned long long)(wall_clock64() - wr0_);
    for (int i_ = 0; i_ < 10; i_++) w_[6 + i_] = (unsigned long long)(wts_[i_ + 1] > wts_[i_] && wts_[i_] ? wts_[i_ + 1] - wts_[i_] : 0);
    for (int i_ = 0; i_ < 10; i_++) w_[16 + i_] = solo::solo_pt_acc[i_];       // per-phase sums over the sub-steps (SOLO_PT)
    for (int i_ = 10; i_ < 14; i_++) w_[18 + i_] = solo::solo_pt_acc[i_];      // (26, 27: the sweep's counters)
  }
#endif
}

template <typename T, int ROBOT>
__global__ void __launch_bounds__(64)
step_kernel(T* __restrict__ sf, int* __restrict__ si, const T* __restrict__ snf, const int* __restrict__ sni, int M,
            Layout L, int N, EnvParams P, PhysParams<T> pp, const float* __restrict__ actions, Outputs out, int mode) {
  step_body<T, ROBOT>(sf, si, snf, sni, M, L, N, P, pp, actions, out, mode);
}

// Two wavefronts per SIMD: the team-mode workgroup (one wavefront, 4 envs) needs 18.4 KB of LDS, so 8 fit a CU, and the
// register budget is held to 256 (the heaviest sweep variants then keep a few callee-saved registers in scratch instead
// of AGPRs).  A lone wavefront issues a VALU instruction every 4 cycles, the SIMD-32 one every 2: above 4096 envs per GPU
// the second wavefront is what fills the issue slots (8192 envs: 0.326 -> 0.27 ms per step; 65 536: 29.5 -> 48.8 M env-steps/s).
// The fp64 instantiation (the reference's arithmetic type; validation precision) is bounded to ONE wavefront per SIMD instead: its
// workgroup needs 37 KB of LDS, so only four fit a CU anyway, and with the 512-entry register budget (256 VGPRs + 256 AGPRs) a value
// that is a register PAIR stops spilling -- measured round 4 (profiles/r04_f64_ab.txt): 1.44 -> 0.55 ms per step at 4096 envs.
#ifndef SOLO_WAVES_PER_SIMD
#define SOLO_WAVES_PER_SIMD 2
#endif
template <typename T, int ROBOT>
__global__ void __launch_bounds__(64, sizeof(T) == 8 ? 1 : SOLO_WAVES_PER_SIMD)
step_kernel_team(T* __restrict__ sf, int* __restrict__ si, const T* __restrict__ snf, const int* __restrict__ sni, int M,
                 Layout L, int N, EnvParams P, PhysParams<T> pp, const float* __restrict__ actions, Outputs out, int mode) {
  step_team<T, ROBOT>(sf, si, snf, sni, M, L, N, P, pp, actions, out, mode);
}

// Helper wavefront: step_kernel_team with a second wavefront per workgroup that runs, in each sub-step, the
// collision front beside the main wavefront's leg dynamics and then the leg sum, the base solve and the leg rates beside its leg
// rows (three workgroup barriers per sub-step: substep_team_helper).  Same grid, same dynamic LDS (the two share the block), same
// register bound; chosen by launch_step while every SIMD can hold both wavefronts of its workgroup.  fp32 only.
template <typename T, int ROBOT>
__global__ void __launch_bounds__(128, SOLO_WAVES_PER_SIMD)
duo_kernel_team(T* __restrict__ sf, int* __restrict__ si, const T* __restrict__ snf, const int* __restrict__ sni, int M,
                Layout L, int N, EnvParams P, PhysParams<T> pp, const float* __restrict__ actions, Outputs out, int mode) {
  static_assert(sizeof(T) == 4, "the helper wavefront is an fp32 kernel");
  step_team<T, ROBOT, true>(sf, si, snf, sni, M, L, N, P, pp, actions, out, mode);
}

// K control steps in one launch (solorl_step_n, solorl_rollout): each wavefront runs step_team K times for its own four envs, and no
// wavefront waits for another between steps.  One launch of step_kernel_team lasts as long as its slowest wavefront, ~2x the mean at
// 4096 envs (profiles/r04_wave_hist.txt); a wavefront's K steps add up to a sum that spreads much less than one step does, so the tail
// costs about one step per window instead of one per step.  Same grid, block and register bound as step_kernel_team; the state still
// makes its HBM round trip every step.  Step k reads actions row k and writes row k of every per-step output ([K][N] rows, offsets in
// 64 bits); ep_stats accumulates as it does over K launches.  With a policy tail (out.pol.value != null, fp32) step k writes row k + 1
// of pol.action / value / logp and reads row k + 1 of pol.noise -- pol.action may be `actions` itself (solorl_rollout: the tail of step
// k writes the action that step k + 1 reads, on the same lane) -- and the last step has no tail unless pol_last.
template <typename T> struct RolloutArgs {
  T* sf; int* si; const T* snf; const int* sni; int M;
  Layout L; int N; EnvParams P; PhysParams<T> pp;
  const float* actions; Outputs out;
  int mode;            // (MODE_STEP, but a kernel argument: a constant would fold step_team's branches differently from step_kernel_team's)
  int K, pol_last;
};
template <typename T> SD T* row_adv(T* p, size_t n) { return p ? p + n : p; }
template <typename T, int ROBOT>
__global__ void __launch_bounds__(64, sizeof(T) == 8 ? 1 : SOLO_WAVES_PER_SIMD)
rollout_kernel_team(const RolloutArgs<T> args) {
  using RA = RolloutArgs<T>;
  typedef const __attribute__((address_space(4))) char* kptr;
  constexpr size_t A = Robot<ROBOT>::NQ;
  const int K = args.K;
#pragma unroll 1
  for (int k = 0; k < K; k++) {
    // the arguments through a pointer the compiler cannot prove loop-invariant: each is loaded where step_team uses it, as in
    // step_kernel_team.  (Read as kernel parameters, all of them were hoisted out of the loop and held across it: 150 spilled VGPRs.)
    kptr ap = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ap));
    const RA& a = *(const RA*)ap;
    const size_t r = (size_t)k * (size_t)a.N, O = (size_t)(a.L.D * (1 + a.L.H));
    Outputs o = a.out;
    o.obs += r * O; o.rew += r; o.done += r;
    o.timeout = row_adv(o.timeout, r); o.success = row_adv(o.success, r); o.nan_reset = row_adv(o.nan_reset, r);
    o.ep_len = row_adv(o.ep_len, r); o.ep_rew = row_adv(o.ep_rew, r); o.goals = row_adv(o.goals, r);
    o.dr0 = row_adv(o.dr0, r); o.dr1 = row_adv(o.dr1, r); o.dr2 = row_adv(o.dr2, r); o.dr3 = row_adv(o.dr3, r); o.dr4 = row_adv(o.dr4, r);
    o.tau = row_adv(o.tau, r * A);
    if (o.pol.value) {                       // (uniform: kernel arguments and the loop counter)
      if (k + 1 < K || a.pol_last) {
        const size_t r1 = r + (size_t)a.N;
        o.pol.value += r1; o.pol.logp += r1; o.pol.action += r1 * A; o.pol.noise = row_adv(o.pol.noise, r1 * A);
      } else o.pol.value = nullptr;
    }
    step_team<T, ROBOT>(a.sf, a.si, a.snf, a.sni, a.M, a.L, a.N, a.P, a.pp, a.actions + r * A, o, a.mode);
    // Between launches the kernel boundary ordered every hand-off from one lane to another; here the next step's reads must stay
    // behind this step's writes: a reset stores state field f on lane f mod 16 and the next step loads the impulse cache, the env
    // scalars and the history on other lanes (those blocks do not start on a multiple of 16), history levels 3 and 4 are shifted in
    // HBM, and the policy tail's activations live in the row storage the next step's sweep rebuilds.
    TEAM_SYNC();
  }
}

// solorl_reset (MASKED = false; mask is null and not read) and solorl_reset_masked (the envs whose mask byte is set; same draws from
// the env's own Philox counter)
template <typename T, int ROBOT, bool MASKED>
__global__ void reset_kernel(T* sf, int* si, const T* snf, const int* sni, int M, Layout L, int N, EnvParams P, float* obs,
                             const unsigned char* mask) {
  const idx_t e = (idx_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (idx_t)N) return;
  if constexpr (MASKED) { if (!mask[si[SX(I_ENVID, e, NI)]]) return; }      // (in front of the state's loads)
  Env<T, Robot<ROBOT>::NQ> E;
  load_env(E, sf, si, L, (idx_t)N, e);
  const idx_t env = (idx_t)si[SX(I_ENVID, e, NI)];
  reset_from_snapshot<T, ROBOT>(E, sf, L, (idx_t)N, e, env, snf, sni, M, P);
  if (obs) write_obs<T, ROBOT>(E, sf, L, (idx_t)N, e, env, P.task, obs);
  store_env(E, sf, si, L, (idx_t)N, e);
  si[SX(I_NEEDRESET, e, NI)] = 0;
}

template <typename T, int ROBOT>
__global__ void obs_kernel(const T* sf, const int* si, Layout L, int N, int task, float* obs) {
  const idx_t e = (idx_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (idx_t)N) return;
  Env<T, Robot<ROBOT>::NQ> E;
  load_env(E, sf, si, L, (idx_t)N, e);
  write_obs<T, ROBOT>(E, sf, L, (idx_t)N, e, (idx_t)si[SX(I_ENVID, e, NI)], task, obs);
}

// solorl_restart_history: every history level the handle uses <- current_state of the state the env holds, for the envs whose mask byte
// is set (read through the slot -> env map, as reset_kernel<.., true> does), then the env's observation row as write_obs lays it out:
// the state words, and per level cs - level = cs - cs, exactly 0 (NaN where cs is not finite, as write_obs gives).  ONE current_state
// feeds the levels and the row.  A second copy behind the stores (write_obs's own) was merged with the first one only in part, and with
// its products shared between the copies the compiler fused other multiply-adds than it does in obs_kernel: the yaw word of one env in 65
// came out 1 ulp from solorl_get_observation's.  Nothing else of the env is written.  (Launched with 256 threads and bounded so.)
template <typename T, int ROBOT>
__global__ void __launch_bounds__(256) restart_history_kernel(T* sf, const int* si, Layout L, int N, int task, float* obs, const unsigned char* mask) {
  const idx_t e = (idx_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (idx_t)N) return;
  const idx_t env = (idx_t)si[SX(I_ENVID, e, NI)];
  if (!mask[env]) return;                                  // (in front of the state's loads)
  Env<T, Robot<ROBOT>::NQ> E;
  load_env(E, sf, si, L, (idx_t)N, e);
  T cs[DMAX];
  current_state<T, ROBOT>(E, task, cs);
  float* o = obs ? obs + env * (idx_t)(L.D * (1 + L.H)) : nullptr;
#pragma unroll
  for (int d = 0; d < DMAX; d++)
    if (d < L.D) {
      for (int h = 0; h < L.H; h++) sf[SX(L.hist + h * HSTRIDE + d, e, L.NF)] = cs[d];
      if (o) {
        o[d] = (float)cs[d];
        for (int h = 0; h < L.H; h++) o[(h + 1) * L.D + d] = (float)(cs[d] - cs[d]);
      }
    }
}

// initial pose of SoloBase.robot_specific_reset (solo.py:291-296) for every env of a buffer
template <typename T>
__global__ void init_pose_kernel(T* sf, int* si, Layout L, int N, T tmy) {
  const idx_t e = (idx_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (idx_t)N) return;
  for (int f = 0; f < L.NF; f++) sf[SX(f, e, L.NF)] = T(0);
  sf[SX(L.pos + 2, e, L.NF)] = T(0.35);
  sf[SX(L.quat + 3, e, L.NF)] = T(1);
  sf[SX(L.tmy, e, L.NF)] = tmy;
  for (int k = 0; k < NI; k++) si[SX(k, e, NI)] = 0;
  si[SX(I_NEEDRESET, e, NI)] = 1;
  si[SX(I_ENVID, e, NI)] = (int)e;
}

template <typename T>
__global__ void copy_env_kernel(const T* sf, const int* si, int N, int src, T* df, int* di, int M, int dst, int NF) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < NF) df[SX(f, (idx_t)dst, NF)] = sf[SX(f, (idx_t)src, NF)];
  if (f < NI) di[SX(f, (idx_t)dst, NI)] = si[SX(f, (idx_t)src, NI)];
}

// ---- contact-count sorting (divergence control for the PGS sweep)
// A PGS sweep costs a wave the MAXIMUM row count over its lanes.  Under a random policy the mean is
// ~4 rows but the maximum over 64 arbitrary envs ~16, so the state is kept physically sorted by the
// last contact count: a stable counting sort (9 buckets, one workgroup) yields perm[dst] = src and a
// gather kernel moves every state field (coalesced writes).  Lanes are independent, so the
// permutation never changes results -- only which envs share a wavefront.
__global__ void __launch_bounds__(256) sort_perm_kernel(const int* __restrict__ si, int N, int* __restrict__ perm) {
  __shared__ int cnt[256][9];
  __shared__ int base[9];
  const int t = threadIdx.x, nt = blockDim.x;
  const int chunk = (N + nt - 1) / nt, lo = t * chunk, hi = lo + chunk < N ? lo + chunk : N;
  int c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = lo; i < hi; i++) { int k = __popc(si[SX(I_MASK, (idx_t)i, NI)] & 0xFFFFFF); k = k > 8 ? 8 : k; c[k]++; }
#pragma unroll
  for (int k = 0; k < 9; k++) cnt[t][k] = c[k];
  __syncthreads();
  if (t < 9) {   // exclusive scan over threads for bucket t (serial: 256 adds)
    int run = 0;
    for (int j = 0; j < nt; j++) { int v = cnt[j][t]; cnt[j][t] = run; run += v; }
    base[t] = run;
  }
  __syncthreads();
  if (t == 0) { int run = 0; for (int k = 0; k < 9; k++) { int v = base[k]; base[k] = run; run += v; } }
  __syncthreads();
  int off[9];
#pragma unroll
  for (int k = 0; k < 9; k++) off[k] = base[k] + cnt[t][k];
  for (int i = lo; i < hi; i++) {
    int k = __popc(si[SX(I_MASK, (idx_t)i, NI)] & 0xFFFFFF); k = k > 8 ? 8 : k;
    int d = 0;
#pragma unroll
    for (int q = 0; q < 9; q++) if (q == k) d = off[q]++;
    perm[d] = i;
  }
}

template <typename T>
__global__ void gather_state_kernel(const T* __restrict__ sf, const int* __restrict__ si, const int* __restrict__ perm, int N,
                                    int NF, T* __restrict__ df, int* __restrict__ di) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const int src = perm[j];
  const int f = blockIdx.y;
  if (f < NF) df[SX(f, (idx_t)j, NF)] = sf[SX(f, (idx_t)src, NF)];
  else di[SX(f - NF, (idx_t)j, NI)] = si[SX(f - NF, (idx_t)src, NI)];
}

// ---- batched state access (solorl_get_states / solorl_set_states): the whole batch as [N] rows of solorl_env_state on the device
// The two sides of the copy have different shapes: the state is AoSoA-4 (SX: a slot group is one contiguous block of NF x 4 values),
// a row is 255 eight-byte words.  A thread per env walking its row would put 2040 B between neighbouring lanes on every row access
// (one 64-B sector per lane and instruction), so: one workgroup per slot group, the group's block staged in LDS; on the state side the
// lanes walk the block itself (whole [field][4] sectors), on the row side they stride over the 4 x 255 words of the group's four rows
// -- consecutive words of a row, and with linear ids of four adjacent rows.  What a word is comes from a 255-entry table the host
// builds once per handle from its Layout (build_state_table): bits 0..15 = a state field, or one of the codes below; bits 16..23 = the
// SOLORL_SF_* group(s) it belongs to.  Entries 256.. of the same array: the group of every state FIELD (xyprev: POSE), which selects
// what the set kernel writes back.  The static LDS below is these kernels' own (the step kernels' rule is per kernel, check_lds_base).
constexpr int ST_WORDS = sizeof(solorl_env_state) / 8;      // 255: 253 doubles + four int32
constexpr int ST_MAXNF = 256;                               // largest Layout::NF (Solo12, four history levels); solorl_create checks
enum : unsigned { ST_ZERO = 0xFFFFu, ST_INT_A = 0xFFFEu /* timestep, need_reset */, ST_INT_B = 0xFFFDu /* contact_mask, rng_counter */ };
static_assert(sizeof(solorl_env_state) == 8 * ST_WORDS && ST_WORDS <= 256, "rows are walked as 8-byte words");

// env id (= row) of the group's slot t, or -1 where the slot lies beyond N or its env is masked out: such a row is never touched
SD int state_row_of(const int* gi, unsigned g, unsigned t, int N, int linear_ids, const unsigned char* mask) {
  const unsigned slot = 4u * g + t;
  if (slot >= (unsigned)N) return -1;
  const int env = linear_ids ? (int)slot : gi[(I_ENVID << 2) + t];
  return (mask && !mask[env]) ? -1 : env;
}
SD void state_word_of(int k, int& s, int& w) { s = (k >= ST_WORDS) + (k >= 2 * ST_WORDS) + (k >= 3 * ST_WORDS); w = k - ST_WORDS * s; }

template <typename T>
__global__ void __launch_bounds__(256) get_states_kernel(const T* __restrict__ sf, const int* __restrict__ si, int NF, int N, int linear_ids,
                                                         const unsigned* __restrict__ tab, const unsigned char* __restrict__ mask,
                                                         unsigned long long* __restrict__ out) {
  __shared__ T stage[ST_MAXNF * 4];
  __shared__ int ints[NI * 4];
  __shared__ int rowof[4];
  const unsigned g = blockIdx.x, t = threadIdx.x;
  const T* gf = sf + (size_t)g * (size_t)(NF << 2);
  const int* gi = si + (size_t)g * (NI << 2);
  if (t < 4) rowof[t] = state_row_of(gi, g, t, N, linear_ids, mask);
  __syncthreads();
  if ((rowof[0] & rowof[1] & rowof[2] & rowof[3]) < 0) return;      // no row of this group is wanted (the whole workgroup leaves): a read of a few envs loads only their groups
  for (int k = t; k < (NF << 2); k += 256) stage[k] = gf[k];
  if (t < NI * 4) ints[t] = gi[t];
  __syncthreads();
  for (int k = t; k < 4 * ST_WORDS; k += 256) {
    int s, w; state_word_of(k, s, w);
    const int env = rowof[s];
    if (env < 0) continue;
    const unsigned code = tab[w] & 0xFFFFu;
    unsigned long long bits = 0ull;                       // ST_ZERO: tau, joints / history levels the handle does not have
    if (code < ST_INT_B) bits = (unsigned long long)__double_as_longlong((double)stage[(code << 2) + s]);
    else if (code == ST_INT_A) bits = (unsigned)ints[(I_TIMESTEP << 2) + s] | ((unsigned long long)(unsigned)ints[(I_NEEDRESET << 2) + s] << 32);
    else if (code == ST_INT_B) bits = (unsigned)ints[(I_MASK << 2) + s] | ((unsigned long long)(unsigned)ints[(I_RNG << 2) + s] << 32);
    out[(size_t)env * ST_WORDS + w] = bits;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) set_states_kernel(T* __restrict__ sf, int* __restrict__ si, int NF, int N, int linear_ids,
                                                         const unsigned* __restrict__ tab, const unsigned char* __restrict__ mask,
                                                         const unsigned long long* __restrict__ in, unsigned fields, int xyprev) {
  __shared__ T stage[ST_MAXNF * 4];
  __shared__ int ints[NI * 4];
  __shared__ int rowof[4];
  const unsigned g = blockIdx.x, t = threadIdx.x;
  T* gf = sf + (size_t)g * (size_t)(NF << 2);
  int* gi = si + (size_t)g * (NI << 2);
  if (t < 4) rowof[t] = state_row_of(gi, g, t, N, linear_ids, mask);
  __syncthreads();
  // rows -> the group's block in LDS: only the words of selected groups of selected rows are read
  for (int k = t; k < 4 * ST_WORDS; k += 256) {
    int s, w; state_word_of(k, s, w);
    const int env = rowof[s];
    if (env < 0) continue;
    const unsigned e = tab[w];
    if (!((e >> 16) & fields)) continue;                  // (ST_ZERO entries belong to no group)
    const unsigned code = e & 0xFFFFu;
    const unsigned long long bits = in[(size_t)env * ST_WORDS + w];
    if (code < ST_INT_B) {
      const T v = (T)__longlong_as_double((long long)bits);
      stage[(code << 2) + s] = v;
      if (w < 2) stage[((xyprev + w) << 2) + s] = v;      // pos x, y are a row's words 0, 1: xyprev = pos xy, as solorl_set_state
    } else if (code == ST_INT_A) {
      ints[(I_TIMESTEP << 2) + s] = (int)(unsigned)bits; ints[(I_NEEDRESET << 2) + s] = (int)(unsigned)(bits >> 32);
    } else {                                              // contact_mask (CONTACT) and rng_counter (COUNTERS) share a word
      if (fields & SOLORL_SF_CONTACT) ints[(I_MASK << 2) + s] = (int)(unsigned)bits;
      if (fields & SOLORL_SF_COUNTERS) ints[(I_RNG << 2) + s] = (int)(unsigned)(bits >> 32);
    }
  }
  __syncthreads();
  // LDS -> state: exactly the elements written above (same selection, by field), in the block's own order
  const unsigned* ftab = tab + 256;
  for (int k = t; k < (NF << 2); k += 256)
    if (rowof[k & 3] >= 0 && (ftab[k >> 2] & fields)) gf[k] = stage[k];
  if (t < NI * 4) {
    const unsigned kk = t >> 2;
    const unsigned grp = kk == I_MASK ? SOLORL_SF_CONTACT : (kk == I_ENVID ? 0u : SOLORL_SF_COUNTERS);
    if (rowof[t & 3] >= 0 && (grp & fields)) gi[t] = ints[t];
  }
}
static_assert(offsetof(solorl_env_state, pos) == 0, "set_states_kernel derives xyprev from a row's words 0 and 1");

// ---- device-side kicks (solorl_perturb; the draws are perturb.hpp's): one thread per storage slot.  The six velocity fields of a slot
// group are [field][4] blocks (SX), so neighbouring threads read and write neighbouring words; countdown / kicks / kick_out are indexed
// by ENV id (the slot's own number, or under contact-count sorting the id the slot carries, as the state kernels read it).  An env that
// is not kicked has no state word loaded or stored; of a kicked one only the components with a non-zero amplitude are.
template <typename T>
__global__ void __launch_bounds__(256) perturb_kernel(T* __restrict__ sf, const int* __restrict__ si, int NF, int N, int linear_ids, int fv, int fw,
                                                      PerturbParams pp, int* __restrict__ countdown, unsigned* __restrict__ kicks,
                                                      double* __restrict__ kick_out) {
  const unsigned slot = blockIdx.x * 256u + threadIdx.x;
  if (slot >= (unsigned)N) return;
  const unsigned env = linear_ids ? slot : (unsigned)si[SX(I_ENVID, slot, NI)];
  if (env >= (unsigned)N) return;
  double kick[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int c = countdown[env] - 1;
  if (c <= 0) {
    const unsigned j = kicks[env];
    c = perturb_kick(pp, pp.id0 + (long long)env, j, kick);
    kicks[env] = j + 1u;
#pragma unroll
    for (int k = 0; k < 6; k++)
      if (pp.max_vel[k] != 0.0) {
        const idx_t at = SX((k < 3 ? fv : fw - 3) + k, slot, NF);
        sf[at] = (T)((double)sf[at] + kick[k]);
      }
  }
  countdown[env] = c;
  if (kick_out) {
#pragma unroll
    for (int k = 0; k < 6; k++) kick_out[(size_t)env * 6 + k] = kick[k];
  }
}

__global__ void __launch_bounds__(256) perturb_state_kernel(const int* __restrict__ countdown, const unsigned* __restrict__ kicks, int N,
                                                            int* __restrict__ countdown_out, unsigned* __restrict__ kicks_out) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)N) return;
  if (countdown_out) countdown_out[i] = countdown[i];
  if (kicks_out) kicks_out[i] = kicks[i];
}

// ---- fused GAE / discounted returns (agents/ppo/storage.py:35-55): one thread per env walks the rollout
// backwards; every access is coalesced across envs.  HBM-bound: 16 B per (t, env) sample.
__global__ void returns_kernel(const float* __restrict__ rew, float* __restrict__ val, const float* __restrict__ msk,
                               const float* __restrict__ nextv, float* __restrict__ ret, int T, int N, int use_gae,
                               float gamma, float lam) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const size_t S = (size_t)N;
  if (use_gae) {
    float vnext = nextv[n];
    val[(size_t)T * S + n] = vnext;
    float gae = 0.f;
#pragma unroll 8
    for (int t = T - 1; t >= 0; t--) {
      const float m = msk[(size_t)(t + 1) * S + n], v = val[(size_t)t * S + n];
      const float delta = rew[(size_t)t * S + n] + gamma * vnext * m - v;
      gae = delta + gamma * lam * m * gae;
      ret[(size_t)t * S + n] = gae + v;
      vnext = v;
    }
  } else {
    float r = nextv[n];
    ret[(size_t)T * S + n] = r;
#pragma unroll 8
    for (int t = T - 1; t >= 0; t--) {
      r = r * gamma * msk[(size_t)(t + 1) * S + n] + rew[(size_t)t * S + n];
      ret[(size_t)t * S + n] = r;
    }
  }
}

// ---- the same walk with time-limit bootstrapping (include/solorl.h solorl_compute_returns_tl): where an episode ended (m == 0) at
// the time limit (tout != 0) the successor's term is the value of the observation the action was taken from, V_t, with weight 1
// instead of V_{t+1} m.  The two operands are selected, the expressions are returns_kernel's: a sample that is no truncation gets
// its bits.  The flag is consulted only where m == 0.  17 B per (t, env) sample (GAE; 16 B without, where the plain walk reads no values).
__global__ void returns_tl_kernel(const float* __restrict__ rew, float* __restrict__ val, const float* __restrict__ msk,
                                  const unsigned char* __restrict__ tout, const float* __restrict__ nextv, float* __restrict__ ret,
                                  int T, int N, int use_gae, float gamma, float lam) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const size_t S = (size_t)N;
  if (use_gae) {
    float vnext = nextv[n];
    val[(size_t)T * S + n] = vnext;
    float gae = 0.f;
#pragma unroll 8
    for (int t = T - 1; t >= 0; t--) {
      const float m = msk[(size_t)(t + 1) * S + n], v = val[(size_t)t * S + n];
      const bool tl = (m == 0.f) & (tout[(size_t)t * S + n] != 0);
      const float boot = tl ? v : vnext, w = tl ? 1.f : m;
      const float delta = rew[(size_t)t * S + n] + gamma * boot * w - v;
      gae = delta + gamma * lam * m * gae;
      ret[(size_t)t * S + n] = gae + v;
      vnext = v;
    }
  } else {
    float r = nextv[n];
    ret[(size_t)T * S + n] = r;
#pragma unroll 8
    for (int t = T - 1; t >= 0; t--) {
      // The value row is read at every step (16 B per sample), not under `if (tl)` (13 B): a load behind a branch keeps the unrolled
      // loop from issuing the next steps' loads ahead.  -DSOLO_RETURNS_TL_BRANCH_LOAD builds that form for the A/B of
      // tools/dev/bench_timelimit.py --variant (profiles/r26_timelimit.json "variants"); the product never defines it.
#ifdef SOLO_RETURNS_TL_BRANCH_LOAD
      const float m = msk[(size_t)(t + 1) * S + n];
      const bool tl = (m == 0.f) & (tout[(size_t)t * S + n] != 0);
      if (tl) r = val[(size_t)t * S + n];
      r = r * gamma * (tl ? 1.f : m) + rew[(size_t)t * S + n];
#else
      const float m = msk[(size_t)(t + 1) * S + n], v = val[(size_t)t * S + n];
      const bool tl = (m == 0.f) & (tout[(size_t)t * S + n] != 0);
      r = (tl ? v : r) * gamma * (tl ? 1.f : m) + rew[(size_t)t * S + n];
#endif
      ret[(size_t)t * S + n] = r;
    }
  }
}

// ---- fused clipped-surrogate PPO loss (agents/ppo/ppo.py:52-74 + the diagonal-Gaussian log-prob / entropy of
// agents/ppo/policy.py:51-58,171-173): forward AND the gradients w.r.t. the network heads in one pass over a
// mini-batch.  One thread per sample; per-block partial sums (deterministic: reduced by the caller), layout
//   part[block][0..2] = sum value-loss, sum action-loss, sample count;  part[block][3 .. 3+A) = d loss / d logstd.
// Sub-gradient conventions are torch's: minimum/maximum split ties evenly, clamp passes the gradient on its
// closed interval -- with both branches equal on a tie the result is the plain derivative.
__global__ void __launch_bounds__(256)
ppo_loss_kernel(const float* __restrict__ mean, const float* __restrict__ logstd, const float* __restrict__ values,
                const float* __restrict__ action, const float* __restrict__ old_logp, const float* __restrict__ adv,
                const float* __restrict__ vpred, const float* __restrict__ ret, int m, int A, float clip, float value_coef,
                int clipped_value, float* __restrict__ g_mean, float* __restrict__ g_values, float* __restrict__ part) {
  extern __shared__ float red[];                  // [256][3 + A] would not fit for large A: reduce column by column
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool on = i < m;
  const float inv_m = 1.0f / (float)m;
  float vl = 0.f, al = 0.f, glp = 0.f;
  float lp = 0.f;
  if (on) {
    for (int j = 0; j < A; j++) {
      const float ls = logstd[j];
      const float z = (action[(size_t)i * A + j] - mean[(size_t)i * A + j]) * __expf(-ls);
      lp += -0.5f * z * z - ls - 0.91893853320467274178f;
    }
    const float ratio = __expf(lp - old_logp[i]);
    const float a = adv[i];
    const float s1 = ratio * a;
    const float rc = fminf(fmaxf(ratio, 1.0f - clip), 1.0f + clip);
    const float s2 = rc * a;
    al = -fminf(s1, s2);
    const float inside = (ratio >= 1.0f - clip && ratio <= 1.0f + clip) ? 1.0f : 0.0f;
    // d min(s1, s2) / d logp:  s1 branch = a*ratio, s2 branch = a*ratio*inside
    const float w = s1 < s2 ? 1.0f : (s1 > s2 ? inside : 0.5f * (1.0f + inside));
    glp = -a * ratio * w * inv_m;
    const float v = values[i], r = ret[i];
    const float u = v - r;
    float gv;
    if (clipped_value) {
      const float dvp = v - vpred[i];
      const float vc = vpred[i] + fminf(fmaxf(dvp, -clip), clip);
      const float wv = vc - r;
      const float ins = (dvp >= -clip && dvp <= clip) ? 1.0f : 0.0f;
      const float uu = u * u, ww = wv * wv;
      vl = 0.5f * fmaxf(uu, ww);
      gv = uu > ww ? u : (uu < ww ? wv * ins : 0.5f * (u + wv * ins));
    } else { vl = 0.5f * u * u; gv = u; }
    g_values[i] = value_coef * gv * inv_m;
  }
  // block reductions: value loss, action loss, then d/dlogstd per action dim (also writes d/dmean)
  auto block_sum = [&](float x) -> float {
    red[threadIdx.x] = x;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    const float r = red[0];
    __syncthreads();
    return r;
  };
  float* P = part + (size_t)blockIdx.x * (3 + A);
  const float svl = block_sum(vl), sal = block_sum(al);
  if (threadIdx.x == 0) { P[0] = svl; P[1] = sal; P[2] = (float)(min(m - (int)(blockIdx.x * blockDim.x), (int)blockDim.x)); }
  for (int j = 0; j < A; j++) {
    float gls = 0.f;
    if (on) {
      const float e = __expf(-logstd[j]);
      const float z = (action[(size_t)i * A + j] - mean[(size_t)i * A + j]) * e;
      g_mean[(size_t)i * A + j] = glp * z * e;          // d logp / d mean_j = z / sigma
      gls = glp * (z * z - 1.0f);                        // d logp / d logstd_j = z^2 - 1
    }
    const float s = block_sum(gls);
    if (threadIdx.x == 0) P[3 + j] = s;
  }
}

}  // namespace

// ================================================================== host side
struct solorl_env {
  solorl_config cfg;
  int N = 0, device = 0, n = 0, D = 0, O = 0, M = 0;
  bool f64 = false, reset_called = false;
  size_t tsize = 4;
  Layout L;
  void* sf = nullptr; int* si = nullptr; void* snf = nullptr; int* sni = nullptr;
  void* sf2 = nullptr; int* si2 = nullptr; int* perm = nullptr;   // double buffer + permutation for contact-count sorting
  bool sort = true;
  uint64_t seed = 0; int64_t id0 = 0;
  double goal_radius = 2.0;
  double* dyn = nullptr;   // device copy of the mutable parameters (EnvParams::dyn)
  std::vector<unsigned> stab_host;   // row-word / field-group table of a solorl_env_state row (build_state_table): solorl_get_state / solorl_set_state
  unsigned* stab = nullptr;          // its device copy: get_states_kernel / set_states_kernel
  bool spread = true;
  bool team = false;   // 16 lanes per env (set at create: default true)
  int lds_poison_on = 0; unsigned lds_poison = 0;   // SOLORL_POISON_LDS test hook
  int simds = 1024;          // SIMDs of the device (4 per CU): grids up to this size have a SIMD per wavefront
  int pipe_override = -1;    // SOLORL_PGS_PIPE=0/1 (dev A/B)
  int helper_override = -1;  // SOLORL_HELPER_WAVE=0/1: pin the helper wavefront (duo_kernel_team) off / on
  // solorl_set_perturbation: the kick schedule, [N] each, indexed by env id (null: no perturbation set)
  int* pert_countdown = nullptr; unsigned* pert_kicks = nullptr;
  PerturbParams pert{};
};

namespace {

EnvParams make_env_params(const solorl_env* h) {
  EnvParams P;
  const solorl_config& c = h->cfg;
  P.task = c.task; P.control = c.control; P.frame_skip = c.frame_skip; P.episode_length = c.episode_length;
  P.hold_torque = c.hold_torque; P.disable_termination = c.disable_termination;
  P.settle_min = c.settle_min; P.nsettle = c.settle_max - c.settle_min + 1;
  P.seed_lo = (unsigned)h->seed; P.seed_hi = (unsigned)(h->seed >> 32); P.id0 = h->id0;
  P.kp = c.kp; P.kd = c.kd; P.max_torque = c.max_torque; P.reward_dt = c.reward_dt; P.dyn = h->dyn;
  P.lds_poison_on = h->lds_poison_on; P.lds_poison = h->lds_poison;
  P.use_treadmill = c.use_treadmill; P.tm_offset = (float)c.treadmill_offset;
  P.linear_ids = h->sort ? 0 : 1;
  return P;
}

// The phase functions address the dynamic LDS from the constant SOLO_LDS_BASE (dynamics.hpp): true exactly while a step kernel's
// static LDS has that size.  Checked against the loaded code object for every kernel a handle can launch, at create (prepare_kernels).
inline int check_lds_base(const void* kernel) {
  hipFuncAttributes a;
  HIP_TRY(hipFuncGetAttributes(&a, kernel));
  if (a.sharedSizeBytes != (size_t)SOLO_LDS_BASE)
    return fail(SOLORL_ERR_HIP, "step kernel's static LDS size differs from SOLO_LDS_BASE: the phase functions' dynamic-LDS base constant does not hold "
                                "(a -DSOLO_WAVE_TIMING build runs team mode only)");
  return 0;
}

// ---- the launch rules, one function each: launches, solorl_create's checks and solorl_get_property all ask these
// team mode's grid: a workgroup per four envs, a multiple of 8 (XCD-contiguous env ranges, step_team)
inline int team_grid(int N) { return (((N + 3) / 4) + 7) & ~7; }
// Pipelined sweep while every wavefront has a SIMD to itself, plain sweep above that (pgs_team_variant: 8192 envs 0.226 ->
// 0.210 ms per step).  The two are re-associations of the same sums, so an env's last bits depend on which side of h->simds
// workgroups its batch is; SOLORL_PGS_PIPE=1 (or 0) pins one variant for every batch size.  A function of the LAUNCH's N: the
// snapshots are simulated with N = 1 (build_snapshots_t) whatever the handle's batch.
inline bool team_pipe(const solorl_env* h, int N) { return h->pipe_override >= 0 ? h->pipe_override != 0 : team_grid(N) <= h->simds; }
// Helper wavefront (duo_kernel_team): fp32 team mode on a fixed state buffer, while the batch's grid gives every SIMD at most one
// workgroup -- its two wavefronts then have the SIMD's two slots to themselves; SOLORL_HELPER_WAVE=0 pins it off (=1 is checked
// against the same rule at create and refused beyond it).  A function of h->N, not of a launch's N: what solorl_get_property
// "helper_wave" reports is what every launch of the handle takes.
inline bool helper_wave_allowed(const solorl_env* h) { return h->team && !h->f64 && !h->sort && team_grid(h->N) <= h->simds; }
inline bool helper_wave_rule(const solorl_env* h) { return h->helper_override != 0 && helper_wave_allowed(h); }
// solorl_step_n / solorl_rollout take one launch exactly where solorl_step is one team-mode launch on a fixed state buffer
inline bool step_n_one_launch(const solorl_env* h) { return h->team && !h->sort; }

// team mode: grid, LDS bytes, and the physics parameters with the sweep variant of this batch size
template <typename T, int ROBOT>
PhysParams<T> team_launch_shape(const solorl_env* h, int N, dim3& grid, size_t& smem) {
  grid = dim3(team_grid(N));
  using TeamLds = RowLds<T, 4>;
  smem = TeamCtx<T, ROBOT, TeamLds>::bytes;
  static_assert(sizeof(T) == 8 || TeamCtx<T, ROBOT, TeamLds>::bytes <= 20480, "team-mode LDS must allow 8 workgroups per CU (two wavefronts per SIMD)");
  PhysParams<T> pp = make_phys<T>(h->cfg);
  pp.mode = (pp.mode & ~PhysParams<T>::M_PIPE) | (team_pipe(h, N) ? PhysParams<T>::M_PIPE : 0);
  return pp;
}

// Once per handle, at create: the SOLO_LDS_BASE check of every step kernel the handle can launch, and lane mode's dynamic-LDS limit
// (hipFuncSetAttribute is per device; the handle's device is current).  launch_step / launch_rollout only shape and launch.
template <typename T, int ROBOT>
int prepare_kernels(const solorl_env* h) {
  if (int rc = check_lds_base(h->team ? reinterpret_cast<const void*>(step_kernel_team<T, ROBOT>) : reinterpret_cast<const void*>(step_kernel<T, ROBOT>))) return rc;
  if constexpr (sizeof(T) == 4)
    if (helper_wave_rule(h))
      if (int rc = check_lds_base(reinterpret_cast<const void*>(duo_kernel_team<T, ROBOT>))) return rc;
  if (step_n_one_launch(h))
    if (int rc = check_lds_base(reinterpret_cast<const void*>(rollout_kernel_team<T, ROBOT>))) return rc;
  if (!h->team)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(step_kernel<T, ROBOT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)RowLds<T>::bytes(sizeof(T) == 8 ? 32 : 64)));
  return 0;
}

template <typename T, int ROBOT>
int launch_step(solorl_env* h, T* sf, int* si, int N, const float* actions, const Outputs& out, int mode, hipStream_t st) {
  if (h->team) {
    dim3 grid;
    size_t team_smem = 0;
    const PhysParams<T> pp = team_launch_shape<T, ROBOT>(h, N, grid, team_smem);
    if constexpr (sizeof(T) == 4) {
      if (helper_wave_rule(h)) {      // two wavefronts per workgroup
        hipLaunchKernelGGL((duo_kernel_team<T, ROBOT>), grid, dim3(128), team_smem, st, sf, si, (const T*)h->snf, (const int*)h->sni, h->M, h->L, N,
                           make_env_params(h), pp, actions, out, mode);
        HIP_TRY(hipGetLastError());
        return 0;
      }
    }
    hipLaunchKernelGGL((step_kernel_team<T, ROBOT>), grid, dim3(64), team_smem, st, sf, si, (const T*)h->snf, (const int*)h->sni, h->M, h->L, N,
                       make_env_params(h), pp, actions, out, mode);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  const int EPB = RowLds<T>::LANES;
  // small workgroups would be packed several to a CU (sharing its LDS pipe and issue slots) while other
  // CUs idle; asking for (almost) the whole LDS forces one workgroup per CU.
  size_t smem = RowLds<T>::bytes(EPB);
  if (h->spread && (N + EPB - 1) / EPB <= 256) smem = RowLds<T>::bytes(sizeof(T) == 8 ? 32 : 64);
  dim3 grid((N + EPB - 1) / EPB), block(EPB);
  hipLaunchKernelGGL((step_kernel<T, ROBOT>), grid, block, smem, st, sf, si, (const T*)h->snf, (const int*)h->sni, h->M, h->L, N,
                     make_env_params(h), make_phys<T>(h->cfg), actions, out, mode);
  HIP_TRY(hipGetLastError());
  return 0;
}

// K team-mode steps in one launch (rollout_kernel_team); the caller has checked step_n_one_launch(h)
template <typename T, int ROBOT>
int launch_rollout(solorl_env* h, T* sf, int* si, int N, const float* actions, const Outputs& out, int K, int pol_last, hipStream_t st) {
  dim3 grid, block(64);
  RolloutArgs<T> a;
  size_t smem = 0;
  a.pp = team_launch_shape<T, ROBOT>(h, N, grid, smem);
  a.sf = sf; a.si = si; a.snf = (const T*)h->snf; a.sni = (const int*)h->sni; a.M = h->M; a.L = h->L; a.N = N; a.P = make_env_params(h);
  a.actions = actions; a.out = out; a.mode = MODE_STEP; a.K = K; a.pol_last = pol_last;
  hipLaunchKernelGGL((rollout_kernel_team<T, ROBOT>), grid, block, smem, st, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

// ---- translation-unit split (build time only; solorl_amd/build.py).  The step kernels' phase functions are what takes minutes to
// compile, once per (arithmetic type, robot): this file is compiled five times in parallel -- SOLO_TU_PART = 0..3 emit ONE
// instantiation of launch_step, launch_rollout and prepare_kernels each (part = 2 * f64 + solo12, part_index) behind hidden C symbols,
// part 4 the C ABI and every other kernel -- or once with SOLO_TU_PART undefined (everything; the -DSOLO_WAVE_TIMING dev build, whose
// device-side counters must live in one translation unit).  The types below the anonymous namespace are the same source in every part.
#define SOLO_LAUNCH_ARGS solorl_env* h, void* sf, int* si, int N, const float* actions, const void* out, int mode, void* st
// the K-step launch (solorl_step_n / solorl_rollout) of the same instantiation, in the same part
#define SOLO_ROLLOUT_ARGS solorl_env* h, void* sf, int* si, int N, const float* actions, const void* out, int K, int pol_last, void* st
#define SOLO_DECLARE_PART(K_) \
  extern "C" __attribute__((visibility("hidden"))) int solorl_prepare_part##K_(const solorl_env* h); \
  extern "C" __attribute__((visibility("hidden"))) int solorl_launch_part##K_(SOLO_LAUNCH_ARGS); \
  extern "C" __attribute__((visibility("hidden"))) int solorl_rollout_part##K_(SOLO_ROLLOUT_ARGS);
SOLO_DECLARE_PART(0) SOLO_DECLARE_PART(1) SOLO_DECLARE_PART(2) SOLO_DECLARE_PART(3)
#define SOLO_DEFINE_PART(K_, T_, R_) \
  extern "C" int solorl_prepare_part##K_(const solorl_env* h) { return prepare_kernels<T_, R_>(h); } \
  extern "C" int solorl_launch_part##K_(SOLO_LAUNCH_ARGS) { \
    return launch_step<T_, R_>(h, (T_*)sf, si, N, actions, *(const Outputs*)out, mode, (hipStream_t)st); } \
  extern "C" int solorl_rollout_part##K_(SOLO_ROLLOUT_ARGS) { \
    return launch_rollout<T_, R_>(h, (T_*)sf, si, N, actions, *(const Outputs*)out, K, pol_last, (hipStream_t)st); }
#if SOLO_TU_PART == -1 || SOLO_TU_PART == 0
SOLO_DEFINE_PART(0, float, 0)
#endif
#if SOLO_TU_PART == -1 || SOLO_TU_PART == 1
SOLO_DEFINE_PART(1, float, 1)
#endif
#if SOLO_TU_PART == -1 || SOLO_TU_PART == 2
SOLO_DEFINE_PART(2, double, 0)
#endif
#if SOLO_TU_PART == -1 || SOLO_TU_PART == 3
SOLO_DEFINE_PART(3, double, 1)
#endif

#if SOLO_TU_PART == -1 || SOLO_TU_PART == 4        // ---- the C ABI and everything that is not a step kernel
namespace {

// The handle's instantiation as tag values: f(T{}) with T = float or double, f(T{}, robot) with decltype(robot)::value = 0 (Solo8) or 1
// (Solo12) -- for everything but the step kernels (part_index)
template <typename F> auto with_type(const solorl_env* h, F&& f) { return h->f64 ? f(double{}) : f(float{}); }
template <typename F> auto with_instantiation(const solorl_env* h, F&& f) {
  return with_type(h, [&](auto t) {
    return h->cfg.robot == SOLORL_ROBOT_SOLO12 ? f(t, std::integral_constant<int, 1>{}) : f(t, std::integral_constant<int, 0>{});
  });
}

// the step kernels' instantiations live in the other parts: the handle's part, and the three hidden functions of each
int part_index(const solorl_env* h) { return 2 * (h->f64 ? 1 : 0) + (h->cfg.robot == SOLORL_ROBOT_SOLO12 ? 1 : 0); }
constexpr decltype(&solorl_launch_part0) PART_LAUNCH[4] = {solorl_launch_part0, solorl_launch_part1, solorl_launch_part2, solorl_launch_part3};
constexpr decltype(&solorl_rollout_part0) PART_ROLLOUT[4] = {solorl_rollout_part0, solorl_rollout_part1, solorl_rollout_part2, solorl_rollout_part3};
constexpr decltype(&solorl_prepare_part0) PART_PREPARE[4] = {solorl_prepare_part0, solorl_prepare_part1, solorl_prepare_part2, solorl_prepare_part3};

int dispatch_step(solorl_env* h, void* sf, int* si, int N, const float* actions, const Outputs& out, int mode, hipStream_t st) {
  return PART_LAUNCH[part_index(h)](h, sf, si, N, actions, &out, mode, st);
}

int dispatch_rollout(solorl_env* h, const float* actions, const Outputs& out, int K, int pol_last, hipStream_t st) {
  return PART_ROLLOUT[part_index(h)](h, h->sf, h->si, h->N, actions, &out, K, pol_last, st);
}

Outputs make_outputs(float* obs_out, float* reward_out, uint8_t* done_out, const solorl_info_soa* info) {
  Outputs o; memset(&o, 0, sizeof o);
  o.obs = obs_out; o.rew = reward_out; o.done = done_out;
  if (info) {
    o.timeout = info->timeout; o.success = info->success; o.nan_reset = info->nan_reset; o.ep_len = info->episode_length;
    o.ep_rew = info->episode_reward; o.goals = info->goals_reached; o.dr0 = info->dr_stand; o.dr1 = info->dr_joint_pose;
    o.dr2 = info->dr_torque; o.dr3 = info->dr_balance; o.dr4 = info->dr_progress; o.ep_stats = info->ep_stats;
    o.tau = info->applied_torque;
  }
  return o;
}

// the policy tail's prerequisites (solorl_step_act, solorl_rollout)
int check_policy_tail(const solorl_env* h, const solorl_policy_params* p, const char* who) {
  const std::string w(who);
  if (h->f64 || !h->team || h->sort) return fail(SOLORL_ERR_INVALID, w + " needs the fp32 team-mode engine without contact-count sorting (the defaults)");
  if (p->hidden != 64 || p->critic_obs_dim != 0 || p->obs_dim != h->O || p->act_dim != h->n || (h->O & 3) || h->O > 88 || h->L.H > 1)     // (step_team copies history levels 0 and 1 to LDS)
    return fail(SOLORL_ERR_INVALID, w + ": the policy must be the MLP of hidden size 64 on this env's observation / action sizes, obs_dim a multiple of 4 "
                                        "and at most 88 (zero or one history level)");
  const void* ptrs[] = {p->critic_w0, p->critic_b0, p->critic_w1, p->critic_b1, p->critic_w2, p->critic_b2, p->actor_w0, p->actor_b0, p->actor_w1, p->actor_b1,
                        p->mean_w, p->mean_b, p->logstd};
  for (const void* q : ptrs) if (!q) return fail(SOLORL_ERR_INVALID, w + ": null policy parameter pointer");
  const void* vec[] = {p->critic_w0, p->critic_w1, p->critic_w2, p->actor_w0, p->actor_w1, p->mean_w};
  for (const void* q : vec) if (reinterpret_cast<uintptr_t>(q) & 15u) return fail(SOLORL_ERR_INVALID, w + ": weight matrices must be 16-byte aligned (rows are read as float4)");
  return 0;
}

// what every step entry point asks after its own checks, in this order (tests pin which message wins)
int step_ready(const solorl_env* h, const float* actions, const float* obs_out, const float* reward_out, const uint8_t* done_out) {
  if (!h->reset_called) return fail(SOLORL_ERR_STATE, "env.reset() must be called before step");   // baseEnv.py:43
  if (!actions || !obs_out || !reward_out || !done_out) return fail(SOLORL_ERR_INVALID, "null array argument");
  HIP_TRY(hipSetDevice(h->device));
  return 0;
}

PolicyTail make_policy_tail(const solorl_policy_params* p, const float* noise, float* value, float* action, float* logp) {
  return PolicyTail{p->critic_w0, p->critic_b0, p->critic_w1, p->critic_b1, p->critic_w2, p->critic_b2, p->actor_w0, p->actor_b0, p->actor_w1, p->actor_b1,
                    p->mean_w, p->mean_b, p->logstd, noise, value, action, logp};
}

// solorl_reset / solorl_reset_masked
template <bool MASKED> int launch_reset(solorl_env* h, const uint8_t* mask, float* obs_out, void* stream) {
  HIP_TRY(hipSetDevice(h->device));
  const EnvParams P = make_env_params(h);
  with_instantiation(h, [&](auto t, auto robot) {
    using T = decltype(t);
    hipLaunchKernelGGL((reset_kernel<T, decltype(robot)::value, MASKED>), dim3((h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, (T*)h->sf, h->si,
                       (const T*)h->snf, (const int*)h->sni, h->M, h->L, h->N, P, obs_out, mask);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

template <typename T> int build_snapshots_t(solorl_env* h) {
  // one scratch env simulated from the reset pose; its state after k = settle_min..settle_max
  // zero-torque control steps is copied into snapshot slot k - settle_min.
  // With the treadmill the settle depends on which side the strip lies: a second set of snapshots (slots nsettle..) for -offset.
  T* tf = nullptr; int* ti = nullptr;
  HIP_TRY(hipMalloc(&tf, sizeof(T) * h->L.NF * 4)); HIP_TRY(hipMalloc(&ti, sizeof(int) * NI * 4));   // (one slot group)
  Outputs none; memset(&none, 0, sizeof none);
  const int nsettle = h->cfg.settle_max - h->cfg.settle_min + 1;
  for (int side = 0; side < (h->cfg.use_treadmill ? 2 : 1); side++) {
    const T tmy = h->cfg.use_treadmill ? (T)(side == 0 ? h->cfg.treadmill_offset : -h->cfg.treadmill_offset) : T(0);
    hipLaunchKernelGGL(init_pose_kernel<T>, dim3(1), dim3(64), 0, 0, tf, ti, h->L, 1, tmy);
    for (int k = 0; k <= h->cfg.settle_max; k++) {      // (k = 0: the reset pose itself is the snapshot when settle_min = 0)
      int rc = k > 0 ? dispatch_step(h, tf, ti, 1, nullptr, none, MODE_SETTLE, 0) : 0;
      if (rc) return rc;
      if (k >= h->cfg.settle_min)
        hipLaunchKernelGGL(copy_env_kernel<T>, dim3((h->L.NF + 63) / 64), dim3(64), 0, 0, (const T*)tf, (const int*)ti, 1, 0,
                           (T*)h->snf, h->sni, h->M, side * nsettle + k - h->cfg.settle_min, h->L.NF);
    }
  }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipFree(tf)); HIP_TRY(hipFree(ti));
  return 0;
}

// The table of get_states_kernel / set_states_kernel (see there): entry w < 255 says what word w of a solorl_env_state row is -- a state
// field of this handle's Layout, an integer pair, or nothing (reads 0, ignored on write) -- and which SOLORL_SF_* group it belongs to;
// entry 256 + f is the group of state field f.  The members' places come from the struct itself (offsetof).
void build_state_table(const Layout& L, int n, std::vector<unsigned>& tab) {
  tab.assign(512, 0u);
  for (int w = 0; w < 256; w++) tab[w] = ST_ZERO;
  auto put = [&](size_t offset, int count, int field, unsigned group) {
    for (int k = 0; k < count; k++) {
      tab[offset / 8 + k] = (unsigned)(field + k) | (group << 16);
      tab[256 + field + k] = group;
    }
  };
#define ST_PUT(member, count, field, group) put(offsetof(solorl_env_state, member), count, field, group)
  ST_PUT(pos, 3, L.pos, SOLORL_SF_POSE); ST_PUT(quat, 4, L.quat, SOLORL_SF_POSE);
  ST_PUT(lin_vel, 3, L.v, SOLORL_SF_VEL); ST_PUT(ang_vel, 3, L.w, SOLORL_SF_VEL);
  ST_PUT(q, n, L.q, SOLORL_SF_JOINT_POS); ST_PUT(qd, n, L.qd, SOLORL_SF_JOINT_VEL);
  ST_PUT(lambda_prev, NPRIM, L.lam, SOLORL_SF_CONTACT);
  for (int hh = 0; hh < (L.H > 2 ? L.H : 2); hh++)      // the levels the handle stores
    put(offsetof(solorl_env_state, hist) + sizeof(double) * DMAX * hh, DMAX, L.hist + hh * HSTRIDE, SOLORL_SF_HISTORY);
  ST_PUT(goal, 2, L.goal, SOLORL_SF_TASK); ST_PUT(potential, 1, L.pot, SOLORL_SF_TASK); ST_PUT(progress, 1, L.prog, SOLORL_SF_TASK);
  ST_PUT(goals_reached, 1, L.goals, SOLORL_SF_TASK); ST_PUT(env_goals_reached, 1, L.egoals, SOLORL_SF_TASK);
  ST_PUT(dr, 5, L.dr, SOLORL_SF_TASK); ST_PUT(treadmill_y, 1, L.tmy, SOLORL_SF_TASK);
#undef ST_PUT
  tab[256 + L.xyprev] = tab[256 + L.xyprev + 1] = SOLORL_SF_POSE;
  tab[offsetof(solorl_env_state, timestep) / 8] = ST_INT_A | ((unsigned)SOLORL_SF_COUNTERS << 16);
  tab[offsetof(solorl_env_state, contact_mask) / 8] = ST_INT_B | ((unsigned)(SOLORL_SF_CONTACT | SOLORL_SF_COUNTERS) << 16);
}
static_assert(offsetof(solorl_env_state, need_reset) == offsetof(solorl_env_state, timestep) + 4 && offsetof(solorl_env_state, timestep) % 8 == 0 &&
              offsetof(solorl_env_state, rng_counter) == offsetof(solorl_env_state, contact_mask) + 4 && NPRIM <= SOLORL_STATE_MAX_PRIMS,
              "the integer members are two 8-byte words: (timestep, need_reset), (contact_mask, rng_counter)");

int check_cfg(const solorl_config* c) {
  if (!c) return fail(SOLORL_ERR_INVALID, "null config");
  if (c->robot != SOLORL_ROBOT_SOLO8 && c->robot != SOLORL_ROBOT_SOLO12) return fail(SOLORL_ERR_INVALID, "robot must be SOLO8 or SOLO12");
  if (c->task < 0 || c->task > 2) return fail(SOLORL_ERR_INVALID, "task must be stand/walk/pointgoal");
  if (c->control != SOLORL_CONTROL_TORQUE && c->control != SOLORL_CONTROL_PD) return fail(SOLORL_ERR_INVALID, "control must be torque or pd");
  if (c->frame_skip < 1 || c->frame_skip > 64) return fail(SOLORL_ERR_INVALID, "frame_skip out of range");
  if (c->num_history_stack < 0 || c->num_history_stack > SOLORL_STATE_MAX_HISTORY) return fail(SOLORL_ERR_INVALID, "num_history_stack must be 0..4");
  if (c->episode_length < 1) return fail(SOLORL_ERR_INVALID, "episode_length must be >= 1");
  if (c->settle_min < 0 || c->settle_max < c->settle_min || c->settle_max > 64) return fail(SOLORL_ERR_INVALID, "bad settle range");
  if (c->settle_min < c->num_history_stack) return fail(SOLORL_ERR_INVALID, "settle_min must be >= num_history_stack");
  if (c->solver_iterations < 1 || c->solver_iterations > 1000) return fail(SOLORL_ERR_INVALID, "solver_iterations out of range");
  if (!(c->sim_dt > 0) || !(c->goal_radius > 1.0)) return fail(SOLORL_ERR_INVALID, "sim_dt must be > 0 and goal_radius > 1");
  if (c->use_treadmill && !(c->treadmill_half_width > 0 && c->treadmill_friction >= 0)) return fail(SOLORL_ERR_INVALID, "bad treadmill parameters");
  if (!(c->solver_residual_threshold >= 0)) return fail(SOLORL_ERR_INVALID, "solver_residual_threshold must be >= 0");
  if (c->friction_model != SOLORL_FRICTION_PYRAMID && c->friction_model != SOLORL_FRICTION_CONE) return fail(SOLORL_ERR_INVALID, "friction_model must be pyramid or cone");
  if (!(c->contact_erp >= 0 && c->contact_erp <= 1) || !(c->erp >= 0 && c->erp <= 1)) return fail(SOLORL_ERR_INVALID, "erp / contact_erp must lie in [0, 1]");
  if (!(c->collision_margin >= 0 && c->collision_margin <= 0.01)) return fail(SOLORL_ERR_INVALID, "collision_margin must lie in [0, 0.01] m");
  if (c->precision != SOLORL_PRECISION_F32 && c->precision != SOLORL_PRECISION_F64) return fail(SOLORL_ERR_INVALID, "bad precision");
  return 0;
}

}  // namespace

extern "C" {

const char* solorl_last_error(void) { return g_err.c_str(); }
// (the library's other translation units report through the same thread-local message; not part of the ABI)
extern "C" int solorl_fail_(int code, const char* msg) { return fail(code, msg); }

#ifdef SOLO_WAVE_TIMING
extern "C" int solorl_debug_wave_times(unsigned long long* out, int nwaves, int reset) {    // [nwaves][SOLO_WT_FIELDS]
  if (nwaves > solo::SOLO_WT_WAVES) nwaves = solo::SOLO_WT_WAVES;
  if (hipDeviceSynchronize() != hipSuccess) return -3;
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(solo::solo_wave_times), (size_t)nwaves * solo::SOLO_WT_FIELDS * sizeof(unsigned long long)) != hipSuccess) return -3;
  if (reset) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(solo::solo_wave_times)) != hipSuccess || hipMemset(p, 0, sizeof(solo::solo_wave_times)) != hipSuccess) return -3;
  }
  return 0;
}
#endif

int solorl_compute_returns(const float* rewards, float* value_preds, const float* masks, const float* next_value,
                           float* returns, int T, int N, int use_gae, float gamma, float gae_lambda, int device_id,
                           void* stream) {
  if (!rewards || !value_preds || !masks || !next_value || !returns) return fail(SOLORL_ERR_INVALID, "null array argument");
  if (T < 1 || N < 1) return fail(SOLORL_ERR_INVALID, "T and N must be >= 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(SOLORL_ERR_NODEVICE, "no HIP device available (no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(SOLORL_ERR_NODEVICE, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  hipLaunchKernelGGL(returns_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, rewards, value_preds, masks,
                     next_value, returns, T, N, use_gae, gamma, gae_lambda);
  HIP_TRY(hipGetLastError());
  return 0;
}
int solorl_compute_returns_tl(const float* rewards, float* value_preds, const float* masks, const uint8_t* timeouts,
                              const float* next_value, float* returns, int T, int N, int use_gae, float gamma, float gae_lambda,
                              int device_id, void* stream) {
  if (!rewards || !value_preds || !masks || !timeouts || !next_value || !returns)
    return fail(SOLORL_ERR_INVALID, "solorl_compute_returns_tl: null array argument (without timeout flags call solorl_compute_returns)");
  if (T < 1 || N < 1) return fail(SOLORL_ERR_INVALID, "solorl_compute_returns_tl: T and N must be >= 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(SOLORL_ERR_NODEVICE, "no HIP device available (no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(SOLORL_ERR_NODEVICE, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  hipLaunchKernelGGL(returns_tl_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, rewards, value_preds, masks,
                     timeouts, next_value, returns, T, N, use_gae, gamma, gae_lambda);
  HIP_TRY(hipGetLastError());
  return 0;
}
int solorl_ppo_loss(const float* mean, const float* logstd, const float* values, const float* action, const float* old_logp,
                    const float* adv, const float* vpred, const float* ret, int m, int A, float clip, float value_coef,
                    int clipped_value, float* grad_mean, float* grad_values, float* partials, int device_id, void* stream) {
  if (!mean || !logstd || !values || !action || !old_logp || !adv || !vpred || !ret || !grad_mean || !grad_values || !partials)
    return fail(SOLORL_ERR_INVALID, "null array argument");
  if (m < 1 || A < 1) return fail(SOLORL_ERR_INVALID, "m and A must be >= 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(SOLORL_ERR_NODEVICE, "no HIP device available (no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(SOLORL_ERR_NODEVICE, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  hipLaunchKernelGGL(ppo_loss_kernel, dim3((m + 255) / 256), dim3(256), 256 * sizeof(float), (hipStream_t)stream, mean, logstd, values,
                     action, old_logp, adv, vpred, ret, m, A, clip, value_coef, clipped_value, grad_mean, grad_values, partials);
  HIP_TRY(hipGetLastError());
  return 0;
}
const char* solorl_version(void) { return "solorl-hip 0.4 (gfx950)"; }
int solorl_abi_version(void) { return SOLORL_ABI_VERSION; }

int solorl_default_config(solorl_config* c, int robot, int task) {
  if (!c) return fail(SOLORL_ERR_INVALID, "null config");
  memset(c, 0, sizeof *c);
  c->robot = robot; c->task = task; c->control = SOLORL_CONTROL_TORQUE;
  c->frame_skip = 4; c->episode_length = 400; c->num_history_stack = 0;
  c->solver_iterations = 50; c->settle_min = 5; c->settle_max = 11; c->precision = SOLORL_PRECISION_F32;
  c->kp = 5.0; c->kd = 0.2; c->max_torque = 3.0; c->sim_dt = 1.0 / 240.0; c->reward_dt = 1.0 / 60.0; c->gravity = 9.81;
  c->erp = 0.2; c->linear_slop = 1e-5; c->warmstart = 0.0; c->damping = 0.04; c->max_velocity = 100.0;
  c->joint_limit = 10.0; c->goal_radius = 2.0;
  c->use_treadmill = 0; c->treadmill_offset = 0.49; c->treadmill_half_width = 0.5; c->treadmill_friction = 0.5;
  c->solver_residual_threshold = 1e-7;     // PyBullet's solverResidualThreshold (K7), see include/solorl.h
  c->collision_margin = 0.001;
  c->friction_model = SOLORL_FRICTION_CONE; c->contact_erp = 0.08;      // [K] ledger, DESIGN.md section 3 (rounds 1-3: pyramid, 0.2)
  return 0;
}

int solorl_create(const solorl_config* cfg, int num_envs, int device_id, uint64_t seed, int64_t env_id_offset, solorl_env** out) {
  if (!out) return fail(SOLORL_ERR_INVALID, "null out pointer");
  *out = nullptr;
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (num_envs < 1) return fail(SOLORL_ERR_INVALID, "num_envs must be >= 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(SOLORL_ERR_NODEVICE, "no HIP device available (the engine has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(SOLORL_ERR_NODEVICE, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  solorl_env* h = new solorl_env();
  h->cfg = *cfg; h->N = num_envs; h->device = device_id; h->seed = seed; h->id0 = env_id_offset;
  h->n = cfg->robot == SOLORL_ROBOT_SOLO12 ? 12 : 8;
  h->D = 14 + 2 * h->n + (cfg->task == SOLORL_TASK_POINTGOAL ? 4 : 0);
  h->O = h->D * (1 + cfg->num_history_stack);
  h->f64 = cfg->precision == SOLORL_PRECISION_F64; h->tsize = h->f64 ? 8 : 4;
  h->L = make_layout(h->n, h->D, cfg->num_history_stack);
  h->M = (cfg->settle_max - cfg->settle_min + 1) * (cfg->use_treadmill ? 2 : 1);
  h->goal_radius = cfg->goal_radius;
  {
    // Lane mode's waves are kept full (RowLds<T>::LANES envs each).  Measured on MI355X (profiles/r01_notes.md): narrower waves do NOT
    // help -- the kernel's duration is the sequential PGS sweep of the heaviest env, which a narrower wave still has to run, while
    // more waves contend for the LDS/TA pipes.
    if (const char* ev = getenv("SOLORL_SPREAD")) h->spread = atoi(ev) != 0;
    h->team = true;   // measured (tools/dev/bench_n.py): team mode wins at every batch size, 1k .. 262k envs; lane mode: SOLORL_TEAM=0
    if (const char* ev = getenv("SOLORL_TEAM")) h->team = atoi(ev) != 0;
    if (const char* ev = getenv("SOLORL_PGS_PIPE")) h->pipe_override = atoi(ev) != 0;
    if (const char* ev = getenv("SOLORL_HELPER_WAVE")) h->helper_override = atoi(ev) != 0;
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) h->simds = 4 * prop.multiProcessorCount; }
    if (const char* ev = getenv("SOLORL_POISON_LDS")) { h->lds_poison_on = 1; h->lds_poison = (unsigned)strtoul(ev, nullptr, 0); }
  }
  auto cleanup = [&](int code) { solorl_destroy(h); return code; };
  const size_t Np = ((size_t)num_envs + 3) & ~(size_t)3, Mp = ((size_t)h->M + 3) & ~(size_t)3;      // slot groups of 4 (SX)
  if ((unsigned long long)h->L.NF * (unsigned long long)Np >= (1ull << 31) ||
      (unsigned long long)(h->L.D * (1 + h->L.H)) * (unsigned long long)num_envs >= (1ull << 31))
    return cleanup(fail(SOLORL_ERR_INVALID, "num_envs too large for 32-bit element indices"));
  if (hipMalloc(&h->sf, h->tsize * h->L.NF * Np) != hipSuccess) return cleanup(fail(SOLORL_ERR_HIP, "hipMalloc state"));
  if (hipMalloc(&h->si, sizeof(int) * NI * Np) != hipSuccess) return cleanup(fail(SOLORL_ERR_HIP, "hipMalloc istate"));
  if (hipMalloc(&h->snf, h->tsize * h->L.NF * Mp) != hipSuccess) return cleanup(fail(SOLORL_ERR_HIP, "hipMalloc snapshot"));
  if (hipMalloc(&h->sni, sizeof(int) * NI * Mp) != hipSuccess) return cleanup(fail(SOLORL_ERR_HIP, "hipMalloc isnapshot"));
  {
    double dyn0[NDYN] = {h->goal_radius, 0.0, 0.0, 0.0};
    if (hipMalloc(&h->dyn, sizeof dyn0) != hipSuccess) return cleanup(fail(SOLORL_ERR_HIP, "hipMalloc dyn"));
    if (hipMemcpy(h->dyn, dyn0, sizeof dyn0, hipMemcpyHostToDevice) != hipSuccess) return cleanup(fail(SOLORL_ERR_HIP, "hipMemcpy dyn"));
  }
  {
    if (h->L.NF > ST_MAXNF) return cleanup(fail(SOLORL_ERR_INVALID, "state layout wider than the batched state kernels' staging block"));
    std::vector<unsigned>& tab = h->stab_host;
    build_state_table(h->L, h->n, tab);
    if (hipMalloc(&h->stab, sizeof(unsigned) * tab.size()) != hipSuccess) return cleanup(fail(SOLORL_ERR_HIP, "hipMalloc state table"));
    if (hipMemcpy(h->stab, tab.data(), sizeof(unsigned) * tab.size(), hipMemcpyHostToDevice) != hipSuccess) return cleanup(fail(SOLORL_ERR_HIP, "hipMemcpy state table"));
  }
  h->sort = false;   // measured with the team-mode sweep (tools/dev/bench_sort.sh): the sort + gather launches cost more than the
                     // padding they save at every batch size (65 536 envs: 29.5 M vs 23.8 M env-steps/s); SOLORL_SORT=1 enables it
  if (const char* ev = getenv("SOLORL_SORT")) h->sort = atoi(ev) != 0 && num_envs >= 2;
  if (h->helper_override == 1 && !helper_wave_allowed(h))
    return cleanup(fail(SOLORL_ERR_INVALID, "SOLORL_HELPER_WAVE=1 needs the fp32 team-mode engine without contact-count sorting and a batch of at most "
                                            "one workgroup (four envs) per SIMD of the device: " + std::to_string(4 * h->simds) + " envs here"));
  if (h->sort) {
    if (hipMalloc(&h->sf2, h->tsize * h->L.NF * Np) != hipSuccess) return cleanup(fail(SOLORL_ERR_HIP, "hipMalloc state2"));
    if (hipMalloc(&h->si2, sizeof(int) * NI * Np) != hipSuccess) return cleanup(fail(SOLORL_ERR_HIP, "hipMalloc istate2"));
    if (hipMalloc(&h->perm, sizeof(int) * (size_t)num_envs) != hipSuccess) return cleanup(fail(SOLORL_ERR_HIP, "hipMalloc perm"));
  }
  if ((rc = PART_PREPARE[part_index(h)](h))) return cleanup(rc);
  rc = with_type(h, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(init_pose_kernel<T>, dim3((num_envs + 255) / 256), dim3(256), 0, 0, (T*)h->sf, h->si, h->L, num_envs, T(0));
    return build_snapshots_t<T>(h);
  });
  if (rc) return cleanup(rc);
  if (hipDeviceSynchronize() != hipSuccess) return cleanup(fail(SOLORL_ERR_HIP, "device sync after create"));
  *out = h;
  return 0;
}

int solorl_destroy(solorl_env* h) {
  if (!h) return 0;
  hipSetDevice(h->device);
  if (h->sf) hipFree(h->sf);
  if (h->si) hipFree(h->si);
  if (h->snf) hipFree(h->snf);
  if (h->sni) hipFree(h->sni);
  if (h->sf2) hipFree(h->sf2);
  if (h->si2) hipFree(h->si2);
  if (h->perm) hipFree(h->perm);
  if (h->dyn) hipFree(h->dyn);
  if (h->stab) hipFree(h->stab);
  if (h->pert_countdown) hipFree(h->pert_countdown);
  if (h->pert_kicks) hipFree(h->pert_kicks);
  delete h;
  return 0;
}

int solorl_dims(const solorl_env* h, int* obs_dim, int* act_dim, int* num_envs) {
  if (!h) return fail(SOLORL_ERR_INVALID, "null handle");
  if (obs_dim) *obs_dim = h->O;
  if (act_dim) *act_dim = h->n;
  if (num_envs) *num_envs = h->N;
  return 0;
}

int solorl_get_property(const solorl_env* h, const char* name, double* value) {
  if (!h || !name || !value) return fail(SOLORL_ERR_INVALID, "null argument");
  const std::string n(name);
  if (n == "lanes_per_env") *value = h->team ? 16 : 1;
  else if (n == "sweep_variant") {
    if (h->cfg.solver_residual_threshold > 0) *value = 2;
    else if (!h->team) *value = 1;          // (lane mode: one software-pipelined row loop)
    else *value = team_pipe(h, h->N) ? 1 : 0;
  } else if (n == "max_contacts") *value = MAX_CONTACTS;
  else if (n == "max_limit_rows") *value = MAX_LIMITS;
  else if (n == "f64") *value = h->f64 ? 1 : 0;
  else if (n == "sort") *value = h->sort ? 1 : 0;
  else if (n == "step_n_one_launch") *value = step_n_one_launch(h) ? 1 : 0;
  else if (n == "helper_wave") *value = helper_wave_rule(h) ? 1 : 0;
  else return fail(SOLORL_ERR_INVALID, "unknown property: " + n);
  return 0;
}

int solorl_reset(solorl_env* h, float* obs_out, void* stream) {
  if (!h) return fail(SOLORL_ERR_INVALID, "null handle");
  if (int rc = launch_reset<false>(h, nullptr, obs_out, stream)) return rc;
  h->reset_called = true;
  return 0;
}

int solorl_step(solorl_env* h, const float* actions, float* obs_out, float* reward_out, uint8_t* done_out,
                const solorl_info_soa* info, void* stream) {
  if (!h) return fail(SOLORL_ERR_INVALID, "null handle");
  if (int rc = step_ready(h, actions, obs_out, reward_out, done_out)) return rc;
  Outputs o = make_outputs(obs_out, reward_out, done_out, info);
  if (h->sort) {   // re-sort the state by last contact count (stable), into the spare buffer
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sort_perm_kernel, dim3(1), dim3(256), 0, st, (const int*)h->si, h->N, h->perm);
    with_type(h, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(gather_state_kernel<T>, dim3((h->N + 255) / 256, h->L.NF + NI), dim3(256), 0, st, (const T*)h->sf, (const int*)h->si,
                         (const int*)h->perm, h->N, h->L.NF, (T*)h->sf2, h->si2);
    });
    HIP_TRY(hipGetLastError());
    std::swap(h->sf, h->sf2); std::swap(h->si, h->si2);
  }
  return dispatch_step(h, h->sf, h->si, h->N, actions, o, MODE_STEP, (hipStream_t)stream);
}

int solorl_step_act(solorl_env* h, const float* actions, float* obs_out, float* reward_out, uint8_t* done_out, const solorl_info_soa* info,
                    const solorl_policy_params* p, const float* noise, float* value_out, float* action_out, float* logp_out, void* stream) {
  if (!h) return fail(SOLORL_ERR_INVALID, "null handle");
  if (!p || !value_out || !action_out || !logp_out) return fail(SOLORL_ERR_INVALID, "solorl_step_act: null policy argument");
  if (int rc = check_policy_tail(h, p, "solorl_step_act")) return rc;
  if (int rc = step_ready(h, actions, obs_out, reward_out, done_out)) return rc;
  Outputs o = make_outputs(obs_out, reward_out, done_out, info);
  o.pol = make_policy_tail(p, noise, value_out, action_out, logp_out);
  return dispatch_step(h, h->sf, h->si, h->N, actions, o, MODE_STEP, (hipStream_t)stream);
}

// per-step rows of the caller's info block for the host-issued form of solorl_step_n (ep_stats is not a per-step field)
static solorl_info_soa info_row(const solorl_info_soa& in, size_t r, size_t A) {
  solorl_info_soa o = in;
  auto adv = [r](auto* p) { return p ? p + r : p; };
  o.timeout = adv(in.timeout); o.success = adv(in.success); o.nan_reset = adv(in.nan_reset); o.episode_length = adv(in.episode_length);
  o.episode_reward = adv(in.episode_reward); o.goals_reached = adv(in.goals_reached); o.dr_stand = adv(in.dr_stand);
  o.dr_joint_pose = adv(in.dr_joint_pose); o.dr_torque = adv(in.dr_torque); o.dr_balance = adv(in.dr_balance); o.dr_progress = adv(in.dr_progress);
  o.applied_torque = in.applied_torque ? in.applied_torque + r * A : nullptr;
  return o;
}

int solorl_step_n(solorl_env* h, int K, const float* actions, float* obs_out, float* reward_out, uint8_t* done_out, const solorl_info_soa* info,
                  void* stream) {
  if (K < 1) return fail(SOLORL_ERR_INVALID, "solorl_step_n: K must be >= 1");
  if (!h) return fail(SOLORL_ERR_INVALID, "null handle");
  if (int rc = step_ready(h, actions, obs_out, reward_out, done_out)) return rc;
  if (!step_n_one_launch(h)) {
    // lane mode and contact-count sorting have no K-step kernel: K ordinary steps, the same results by construction
    const size_t N = (size_t)h->N, O = (size_t)h->O, A = (size_t)h->n;
    for (int k = 0; k < K; k++) {
      const size_t r = (size_t)k * N;
      solorl_info_soa ik;
      if (info) ik = info_row(*info, r, A);
      if (int rc = solorl_step(h, actions + r * A, obs_out + r * O, reward_out + r, done_out + r, info ? &ik : nullptr, stream)) return rc;
    }
    return 0;
  }
  // (K = 1: the one-step kernel itself, so that a one-step call is solorl_step exactly)
  if (K == 1) return dispatch_step(h, h->sf, h->si, h->N, actions, make_outputs(obs_out, reward_out, done_out, info), MODE_STEP, (hipStream_t)stream);
  return dispatch_rollout(h, actions, make_outputs(obs_out, reward_out, done_out, info), K, 0, (hipStream_t)stream);
}

int solorl_rollout(solorl_env* h, int K, float* actions, float* obs_out, float* reward_out, uint8_t* done_out, const solorl_info_soa* info,
                   const solorl_policy_params* p, const float* noise, float* value_out, float* logp_out, int policy_after_last, void* stream) {
  if (K < 1) return fail(SOLORL_ERR_INVALID, "solorl_rollout: K must be >= 1");
  if (!h) return fail(SOLORL_ERR_INVALID, "null handle");
  if (!p || !value_out || !logp_out) return fail(SOLORL_ERR_INVALID, "solorl_rollout: null policy argument");
  if (int rc = check_policy_tail(h, p, "solorl_rollout")) return rc;
  if (int rc = step_ready(h, actions, obs_out, reward_out, done_out)) return rc;
  Outputs o = make_outputs(obs_out, reward_out, done_out, info);
  o.pol = make_policy_tail(p, noise, value_out, actions, logp_out);
  if (K == 1) {              // = solorl_step_act (policy after the step) or solorl_step, as in solorl_step_n
    if (policy_after_last) { o.pol.value = value_out + h->N; o.pol.logp = logp_out + h->N; o.pol.action = actions + (size_t)h->N * h->n; if (noise) o.pol.noise = noise + (size_t)h->N * h->n; }
    else o.pol = PolicyTail{};
    return dispatch_step(h, h->sf, h->si, h->N, actions, o, MODE_STEP, (hipStream_t)stream);
  }
  return dispatch_rollout(h, actions, o, K, policy_after_last != 0, (hipStream_t)stream);
}

int solorl_get_observation(solorl_env* h, float* obs_out, void* stream) {
  if (!h || !obs_out) return fail(SOLORL_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  with_instantiation(h, [&](auto t, auto robot) {
    using T = decltype(t);
    hipLaunchKernelGGL((obs_kernel<T, decltype(robot)::value>), dim3((h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const T*)h->sf,
                       (const int*)h->si, h->L, h->N, h->cfg.task, obs_out);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

int solorl_increment_curriculum(solorl_env* h, double value) {
  if (!h) return fail(SOLORL_ERR_INVALID, "null handle");
  if (h->cfg.task != SOLORL_TASK_POINTGOAL) return 0;                  // solo.py:332-334 (assert task == 'pointgoal')
  HIP_TRY(hipSetDevice(h->device));
  // The kernels read goal_radius from the handle's device block, so launches already captured in a HIP graph see the
  // new value at their next replay.  Host-synchronising (rare call: once per curriculum_schedule updates): every step
  // enqueued before this call samples with the old radius, every later one with the new.
  HIP_TRY(hipDeviceSynchronize());
  h->goal_radius += value;
  HIP_TRY(hipMemcpy(h->dyn + DYN_GOAL_RADIUS, &h->goal_radius, sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

static int find_slot(solorl_env* h, int env, int* slot) {
  // the state is kept sorted by contact count: look the env up in the slot -> env-id map
  if (!h->sort) { *slot = env; return 0; }
  const size_t Np = ((size_t)h->N + 3) & ~(size_t)3;
  std::vector<int> all(NI * Np);
  HIP_TRY(hipMemcpy(all.data(), h->si, sizeof(int) * NI * Np, hipMemcpyDeviceToHost));
  for (int s = 0; s < h->N; s++) if (all[(size_t)(s >> 2) * (NI << 2) + ((size_t)I_ENVID << 2) + (s & 3)] == env) { *slot = s; return 0; }
  return fail(SOLORL_ERR_INVALID, "env id not found in slot map");
}

int solorl_get_state(solorl_env* h, int i, solorl_env_state* out) {
  if (!h || !out || i < 0 || i >= h->N) return fail(SOLORL_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  { int rc_ = find_slot(h, i, &i); if (rc_) return rc_; }
  // slot i of the AoSoA-4 storage (SX): its fields are 4 elements apart, starting at element (i >> 2) * NF * 4 + (i & 3)
  const size_t slot0f = (size_t)(i >> 2) * ((size_t)h->L.NF << 2) + (size_t)(i & 3), slot0i = (size_t)(i >> 2) * ((size_t)NI << 2) + (size_t)(i & 3);
  std::vector<double> f(h->L.NF);
  int iv[NI];
  if (h->f64) {
    HIP_TRY(hipMemcpy2D(f.data(), sizeof(double), (const char*)h->sf + sizeof(double) * slot0f, sizeof(double) * 4, sizeof(double), h->L.NF, hipMemcpyDeviceToHost));
  } else {
    std::vector<float> ff(h->L.NF);
    HIP_TRY(hipMemcpy2D(ff.data(), sizeof(float), (const char*)h->sf + sizeof(float) * slot0f, sizeof(float) * 4, sizeof(float), h->L.NF, hipMemcpyDeviceToHost));
    for (int k = 0; k < h->L.NF; k++) f[k] = ff[k];
  }
  HIP_TRY(hipMemcpy2D(iv, sizeof(int), (const char*)h->si + sizeof(int) * slot0i, sizeof(int) * 4, sizeof(int), NI, hipMemcpyDeviceToHost));
  memset(out, 0, sizeof *out);            // (words no field maps to read 0: tau, joints / history levels the handle does not have)
  for (int w = 0; w < ST_WORDS; w++) {    // the row's double members, by the table of the batched kernels
    const unsigned code = h->stab_host[w] & 0xFFFFu;
    if (code < ST_INT_B) memcpy(reinterpret_cast<char*>(out) + 8 * w, &f[code], 8);
  }
  out->timestep = iv[I_TIMESTEP]; out->contact_mask = iv[I_MASK]; out->rng_counter = iv[I_RNG]; out->need_reset = iv[I_NEEDRESET];
  return 0;
}

int solorl_set_state(solorl_env* h, int i, const solorl_env_state* in) {
  if (!h || !in || i < 0 || i >= h->N) return fail(SOLORL_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  const int env_id = i;
  { int rc_ = find_slot(h, i, &i); if (rc_) return rc_; }
  const Layout& L = h->L;
  const size_t slot0f = (size_t)(i >> 2) * ((size_t)L.NF << 2) + (size_t)(i & 3), slot0i = (size_t)(i >> 2) * ((size_t)NI << 2) + (size_t)(i & 3);
  std::vector<double> f(L.NF, 0.0);       // (fields no row word maps to are written as 0: pads, joints / history levels the handle does not have)
  for (int w = 0; w < ST_WORDS; w++) {    // the row's double members, by the table of the batched kernels
    const unsigned code = h->stab_host[w] & 0xFFFFu;
    if (code < ST_INT_B) memcpy(&f[code], reinterpret_cast<const char*>(in) + 8 * w, 8);
  }
  f[L.xyprev] = in->pos[0]; f[L.xyprev + 1] = in->pos[1];
  int iv[NI]; iv[I_TIMESTEP] = in->timestep; iv[I_MASK] = in->contact_mask; iv[I_RNG] = in->rng_counter; iv[I_NEEDRESET] = in->need_reset;
  iv[I_ENVID] = env_id;
  if (h->f64) {
    HIP_TRY(hipMemcpy2D((char*)h->sf + sizeof(double) * slot0f, sizeof(double) * 4, f.data(), sizeof(double), sizeof(double), L.NF, hipMemcpyHostToDevice));
  } else {
    std::vector<float> ff(L.NF);
    for (int k = 0; k < L.NF; k++) ff[k] = (float)f[k];
    HIP_TRY(hipMemcpy2D((char*)h->sf + sizeof(float) * slot0f, sizeof(float) * 4, ff.data(), sizeof(float), sizeof(float), L.NF, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy2D((char*)h->si + sizeof(int) * slot0i, sizeof(int) * 4, iv, sizeof(int), sizeof(int), NI, hipMemcpyHostToDevice));
  if (!in->need_reset) h->reset_called = true;
  return 0;
}

// ---- the whole batch's state as one device array (get_states_kernel / set_states_kernel above): no host synchronisation, no
// allocation, no slot lookup on the host -- under contact-count sorting every slot's thread reads its env id, as reset_kernel does
static dim3 state_grid(const solorl_env* h) { return dim3((unsigned)((h->N + 3) / 4)); }

int solorl_get_states(solorl_env* h, const uint8_t* mask, solorl_env_state* out, void* stream) {
  if (!h) return fail(SOLORL_ERR_INVALID, "solorl_get_states: null handle");
  if (!out) return fail(SOLORL_ERR_INVALID, "solorl_get_states: null out array");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  with_type(h, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(get_states_kernel<T>, state_grid(h), dim3(256), 0, st, (const T*)h->sf, (const int*)h->si, h->L.NF, h->N, h->sort ? 0 : 1,
                       (const unsigned*)h->stab, mask, (unsigned long long*)out);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

int solorl_set_states(solorl_env* h, const uint8_t* mask, const solorl_env_state* in, uint32_t fields, void* stream) {
  if (!h) return fail(SOLORL_ERR_INVALID, "solorl_set_states: null handle");
  if (!in) return fail(SOLORL_ERR_INVALID, "solorl_set_states: null in array");
  if (fields == 0 || (fields & ~(uint32_t)SOLORL_SF_ALL)) return fail(SOLORL_ERR_INVALID, "solorl_set_states: fields must be a non-empty set of SOLORL_SF_* bits");
  const bool whole = !mask && fields == (uint32_t)SOLORL_SF_ALL;
  if (!whole && !h->reset_called)
    return fail(SOLORL_ERR_STATE, "solorl_set_states: a partial write (a mask, or fewer than all field groups) needs a handle that has been reset");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  with_type(h, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(set_states_kernel<T>, state_grid(h), dim3(256), 0, st, (T*)h->sf, h->si, h->L.NF, h->N, h->sort ? 0 : 1,
                       (const unsigned*)h->stab, mask, (const unsigned long long*)in, (unsigned)fields, h->L.xyprev);
  });
  HIP_TRY(hipGetLastError());
  if (whole) h->reset_called = true;      // every env now holds a caller-given state (the rows' own need_reset values are the caller's business)
  return 0;
}

int solorl_reset_masked(solorl_env* h, const uint8_t* mask, float* obs_out, void* stream) {
  if (!h) return fail(SOLORL_ERR_INVALID, "solorl_reset_masked: null handle");
  if (!mask) return fail(SOLORL_ERR_INVALID, "solorl_reset_masked: null mask");
  if (!h->reset_called) return fail(SOLORL_ERR_STATE, "solorl_reset_masked: needs a handle that has been reset");
  return launch_reset<true>(h, mask, obs_out, stream);
}

int solorl_restart_history(solorl_env* h, const uint8_t* mask, float* obs_out, void* stream) {
  if (!h) return fail(SOLORL_ERR_INVALID, "solorl_restart_history: null handle");
  if (!mask) return fail(SOLORL_ERR_INVALID, "solorl_restart_history: null mask");
  if (!h->reset_called) return fail(SOLORL_ERR_STATE, "solorl_restart_history: needs a handle that has been reset");
  HIP_TRY(hipSetDevice(h->device));
  with_instantiation(h, [&](auto t, auto robot) {
    using T = decltype(t);
    hipLaunchKernelGGL((restart_history_kernel<T, decltype(robot)::value>), dim3((h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, (T*)h->sf, (const int*)h->si,
                       h->L, h->N, h->cfg.task, obs_out, mask);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- device-side kicks (perturb_kernel above; the draw rules are in include/solorl.h)
int solorl_set_perturbation(solorl_env* h, const solorl_perturbation* p) {
  if (!h) return fail(SOLORL_ERR_INVALID, "solorl_set_perturbation: null handle");
  HIP_TRY(hipSetDevice(h->device));
  if (!p) {                                    // switch off
    if (h->pert_countdown) HIP_TRY(hipFree(h->pert_countdown));
    h->pert_countdown = nullptr;
    if (h->pert_kicks) HIP_TRY(hipFree(h->pert_kicks));
    h->pert_kicks = nullptr;
    return 0;
  }
  if (p->interval_min < 1 || p->interval_max < p->interval_min)
    return fail(SOLORL_ERR_INVALID, "solorl_set_perturbation: the interval must satisfy 1 <= interval_min <= interval_max");
  PerturbParams pp{};
  for (int k = 0; k < 6; k++) {
    const double m = k < 3 ? p->max_lin_vel[k] : p->max_ang_vel[k - 3];
    if (!std::isfinite(m) || m < 0.0) return fail(SOLORL_ERR_INVALID, "solorl_set_perturbation: amplitudes must be finite and >= 0");
    pp.max_vel[k] = m;
  }
  pp.seed_lo = (unsigned)h->seed; pp.seed_hi = (unsigned)(h->seed >> 32); pp.id0 = h->id0;
  pp.interval_min = p->interval_min; pp.span = (unsigned)p->interval_max - (unsigned)p->interval_min + 1u;
  const size_t N = (size_t)h->N;
  if (!h->pert_countdown && hipMalloc(&h->pert_countdown, sizeof(int) * N) != hipSuccess) { h->pert_countdown = nullptr; return fail(SOLORL_ERR_HIP, "solorl_set_perturbation: hipMalloc countdown"); }
  if (!h->pert_kicks && hipMalloc(&h->pert_kicks, sizeof(unsigned) * N) != hipSuccess) { h->pert_kicks = nullptr; return fail(SOLORL_ERR_HIP, "solorl_set_perturbation: hipMalloc kicks"); }
  std::vector<int> first(N);
  for (size_t i = 0; i < N; i++) first[i] = perturb_first_countdown(pp, pp.id0 + (long long)i);
  HIP_TRY(hipDeviceSynchronize());             // (a restart must not overtake perturb launches still in flight on another stream)
  HIP_TRY(hipMemcpy(h->pert_countdown, first.data(), sizeof(int) * N, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(h->pert_kicks, 0, sizeof(unsigned) * N));
  HIP_TRY(hipDeviceSynchronize());
  h->pert = pp;
  return 0;
}

int solorl_perturb(solorl_env* h, double* kick_out, void* stream) {
  if (!h) return fail(SOLORL_ERR_INVALID, "solorl_perturb: null handle");
  if (!h->pert_countdown || !h->pert_kicks) return fail(SOLORL_ERR_STATE, "solorl_perturb: no perturbation set (solorl_set_perturbation)");
  if (!h->reset_called) return fail(SOLORL_ERR_STATE, "solorl_perturb: needs a handle that has been reset");
  HIP_TRY(hipSetDevice(h->device));
  with_type(h, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(perturb_kernel<T>, dim3((unsigned)((h->N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (T*)h->sf, (const int*)h->si, h->L.NF, h->N,
                       h->sort ? 0 : 1, h->L.v, h->L.w, h->pert, h->pert_countdown, h->pert_kicks, kick_out);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

int solorl_get_perturbation(solorl_env* h, int32_t* countdown_out, uint32_t* kicks_out, void* stream) {
  if (!h) return fail(SOLORL_ERR_INVALID, "solorl_get_perturbation: null handle");
  if (!countdown_out && !kicks_out) return fail(SOLORL_ERR_INVALID, "solorl_get_perturbation: null out arrays");
  if (!h->pert_countdown || !h->pert_kicks) return fail(SOLORL_ERR_STATE, "solorl_get_perturbation: no perturbation set (solorl_set_perturbation)");
  HIP_TRY(hipSetDevice(h->device));
  hipLaunchKernelGGL(perturb_state_kernel, dim3((unsigned)((h->N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const int*)h->pert_countdown,
                     (const unsigned*)h->pert_kicks, h->N, (int*)countdown_out, (unsigned*)kicks_out);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
#endif  // SOLO_TU_PART: the C ABI part
