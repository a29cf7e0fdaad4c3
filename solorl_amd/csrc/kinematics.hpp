// kinematics.hpp -- derived quantities of ONE env's state row (include/solorl.h solorl_env_kin): link poses and velocities, the
// collision primitives' support points with their velocities and normal forces, centre of mass, energy and momentum.
//
// One function, env_kinematics<T, ROBOT>, made of five independent parts (the base, the four legs: KinRow) and the sum of their shares.
// solorl_kin.hip runs a row's parts on four wavefronts (a leg each, the base before the first), one lane per env each; tests/host/rows_main.cpp, compiled by g++ under
// SOLO_HOST_SHIM, calls the function as it is.  A row is read through `ld(word)` and written through `st(word, value)`; every word index
// is a compile-time constant after unrolling, so on the device both are LDS accesses at immediate offsets and nothing is indexed
// by data.
//
// The support points are not restated here: the leg primitives come from leg_prim_points (disc_point, ring_disc_point, disc_point_x:
// what phase_detect and the team front call), the base points from the model table as phase_detect reads it.  The frames come from
// leg_frames.  What this file adds is what the step never needs as such: the velocity of every frame (w_i = w_parent + qd_i a_i,
// v_origin_i = v_origin_parent + w_parent x (o_i - o_parent)), the link quaternions (composed from half-angle rotations beside the
// matrices), and the sums over links of the oracle's oracle_energy_momentum.
#pragma once
#include <cstddef>

#include "state_row.hpp"

namespace solo {

constexpr int KIN_OUT_WORDS = sizeof(solorl_env_kin) / 8;         // 455
// the part of a state row that is read: pos .. lambda_prev, one contiguous segment (tau lies inside it and is skipped), and the 8-byte
// word that holds contact_mask
constexpr int KIN_IN_HEAD_WORDS = (offsetof(solorl_env_state, lambda_prev) + sizeof(double) * SOLORL_STATE_MAX_PRIMS) / 8;   // 73
constexpr int KIN_IN_MASK_WORD = offsetof(solorl_env_state, contact_mask) / 8;                                              // 254
constexpr int KIN_IN_WORDS = KIN_IN_HEAD_WORDS + 1;               // staged words per row: the head, then the contact_mask word
static_assert(sizeof(solorl_env_kin) == 3640 && offsetof(solorl_env_state, contact_mask) % 8 == 0, "row layouts of include/solorl.h");
static_assert(SOLORL_KIN_MAX_LINKS == SOLORL_MAX_LINKS && SOLORL_STATE_MAX_PRIMS == NPRIM, "table sizes");

#define KIN_KW(member) ((int)(offsetof(solorl_env_kin, member) / 8))

template <typename T> struct Quat { T x, y, z, w; };
// p (x) rotation by the half-angle pair (ch, sh) about the link's x (AX = 0) or y axis: the quaternion beside rot_axis<AX>
template <int AX, typename T> SD Quat<T> quat_rot_axis(const Quat<T>& p, T ch, T sh) {
  if constexpr (AX == 0) return {p.w * sh + p.x * ch, p.y * ch + p.z * sh, p.z * ch - p.y * sh, p.w * ch - p.x * sh};
  else return {p.x * ch - p.z * sh, p.w * sh + p.y * ch, p.z * ch + p.x * sh, p.w * ch - p.y * sh};
}

// sums over links: kinetic and potential energy, mass, linear momentum, angular momentum about the world origin, mass x COM
template <typename T> struct KinSums { T KE, PE, M; V3<T> P, Lm, MC; };
constexpr int KIN_SUM_WORDS = 12;
// a share as KIN_SUM_WORDS words and back (how the device's wavefronts hand their shares to the one that adds them)
template <typename T> SD void kin_sums_to_words(T* q, const KinSums<T>& A) {
  q[0] = A.KE; q[1] = A.PE; q[2] = A.M; q[3] = A.P.x; q[4] = A.P.y; q[5] = A.P.z;
  q[6] = A.Lm.x; q[7] = A.Lm.y; q[8] = A.Lm.z; q[9] = A.MC.x; q[10] = A.MC.y; q[11] = A.MC.z;
}
template <typename T> SD KinSums<T> kin_sums_from_words(const T* q) {
  return KinSums<T>{q[0], q[1], q[2], mk(q[3], q[4], q[5]), mk(q[6], q[7], q[8]), mk(q[9], q[10], q[11])};
}
constexpr int KIN_PARTS = 5;          // the base with its twelve points, then one part per leg: independent of each other up to the sums

// One state row's work, in KIN_PARTS independent parts: base() or leg<L>() writes that part's members of the output row and leaves its
// share of the link sums in S; kin_totals adds the five shares in a fixed order and writes the totals.  The device runs the parts of a
// row on four wavefronts (the base on the first leg's), the host one after the other: same functions, same order of summation.
// ld(w): word w of the state row (w a member's STATE_SW offset + index);  st(w, v): word w of the solorl_env_kin row.
// cmask: the row's contact_mask;  urdf: solorl_config use_urdf_inertia != 0.
template <typename T, int ROBOT, typename LD, typename ST> struct KinRow {
  using RB = Robot<ROBOT>;
  static constexpr int NJ = RB::NJ, NQ = RB::NQ, NL = RB::NL;
  static_assert(RB::MD.nlinks == NL && RB::MD.nprims == (RB::SHOULDER ? 24 : 20), "model table");
  LD ld; ST st;
  int cmask; bool urdf; T sim_dt, gravity;
  V3<T> pos, v0, w0; M3<T> R0; Quat<T> Q0;
  KinSums<T> S;

  SD KinRow(LD ld_, ST st_, int cmask_, bool urdf_, T sim_dt_, T gravity_) : ld(ld_), st(st_), cmask(cmask_), urdf(urdf_), sim_dt(sim_dt_), gravity(gravity_) {
    pos = mk(ld(STATE_SW(pos)), ld(STATE_SW(pos) + 1), ld(STATE_SW(pos) + 2));
    const T qx = ld(STATE_SW(quat)), qy = ld(STATE_SW(quat) + 1), qz = ld(STATE_SW(quat) + 2), qw = ld(STATE_SW(quat) + 3);
    v0 = mk(ld(STATE_SW(lin_vel)), ld(STATE_SW(lin_vel) + 1), ld(STATE_SW(lin_vel) + 2));
    w0 = mk(ld(STATE_SW(ang_vel)), ld(STATE_SW(ang_vel) + 1), ld(STATE_SW(ang_vel) + 2));
    R0 = quat_to_mat(qx, qy, qz, qw);             // the state's quaternion as it is, as the step reads it
    const T qn = rsqrt_fast(qx * qx + qy * qy + qz * qz + qw * qw);
    Q0 = Quat<T>{qx * qn, qy * qn, qz * qn, qw * qn};
    const V3<T> z = mk(T(0), T(0), T(0));
    S = KinSums<T>{T(0), T(0), T(0), z, z, z};
  }
  SD void st3(int w, V3<T> v) { st(w, v.x); st(w + 1, v.y); st(w + 2, v.z); }

  // one link: frame (R, o relative to the base origin, q), angular velocity w, velocity vo of its origin
  template <int l> SD void link(const M3<T>& R, V3<T> o, const Quat<T>& q, V3<T> w, V3<T> vo) {
    constexpr solorl_link_data LK = RB::MD.links[l];
    const V3<T> rc = addc(mk(T(0), T(0), T(0)), R, LK.com[0], LK.com[1], LK.com[2]);
    const V3<T> c = pos + (o + rc), vc = vo + cross(w, rc);
    st3(KIN_KW(link_pos) + 3 * l, pos + o);
    const bool neg = q.w < T(0);
    st(KIN_KW(link_quat) + 4 * l, neg ? -q.x : q.x); st(KIN_KW(link_quat) + 4 * l + 1, neg ? -q.y : q.y);
    st(KIN_KW(link_quat) + 4 * l + 2, neg ? -q.z : q.z); st(KIN_KW(link_quat) + 4 * l + 3, neg ? -q.w : q.w);
    st3(KIN_KW(link_com) + 3 * l, c);
    st3(KIN_KW(link_com_vel) + 3 * l, vc);
    st3(KIN_KW(link_ang_vel) + 3 * l, w);
    const LinkInertia<T> I = link_inertia<T, ROBOT, l>(urdf);
    const V3<T> wl = mk(dot(R.c0, w), dot(R.c1, w), dot(R.c2, w));
    const V3<T> Iw = mul(R, mk(I.xx * wl.x + I.xy * wl.y + I.xz * wl.z, I.xy * wl.x + I.yy * wl.y + I.yz * wl.z, I.xz * wl.x + I.yz * wl.y + I.zz * wl.z));
    const T m = T(LK.mass);
    S.KE += T(0.5) * m * dot(vc, vc) + T(0.5) * dot(w, Iw);
    S.PE += m * gravity * c.z;
    S.P = fma3(vc, m, S.P);
    S.Lm = fma3(cross(c, vc), m, S.Lm) + Iw;
    S.MC = fma3(c, m, S.MC);
    S.M += m;
    ROW_FENCE();
  }
  // one primitive: support point Pp relative to the base origin, on a link with origin o, angular velocity w, origin velocity vo
  SD void prim(int p, V3<T> Pp, V3<T> o, V3<T> w, V3<T> vo) {
    st3(KIN_KW(prim_point) + 3 * p, pos + Pp);
    st3(KIN_KW(prim_vel) + 3 * p, vo + cross(w, Pp - o));
    // (divided whether in contact or not, then selected: a branch here would split the row's arithmetic into blocks, and the compiler
    // then sinks every link's energy and momentum terms into the last one, with all links' frames live until there)
    const T force = ld(STATE_SW(lambda_prev) + p) / sim_dt;
    st(KIN_KW(prim_force) + p, ((cmask >> p) & 1) ? force : T(0));
    ROW_FENCE();
  }

  // the base link, its twelve points, and the rows a Solo8 does not have (they read 0)
  SD void base() {
    const V3<T> zero = mk(T(0), T(0), T(0));
    link<0>(R0, zero, Q0, w0, v0);
    static_for<12>([&](auto pc) {
      constexpr int p = decltype(pc)::value;
      constexpr solorl_prim_data PR = RB::MD.prims[p];
      static_assert(PR.link == 0 && PR.axis == -1, "base primitives are points");
      prim(p, addc(zero, R0, PR.center[0], PR.center[1], PR.center[2]), zero, w0, v0);
    });
    static_for<SOLORL_KIN_MAX_LINKS - NL>([&](auto ic) {
      constexpr int l = NL + decltype(ic)::value;
      st3(KIN_KW(link_pos) + 3 * l, zero); st3(KIN_KW(link_com) + 3 * l, zero); st3(KIN_KW(link_com_vel) + 3 * l, zero);
      st3(KIN_KW(link_ang_vel) + 3 * l, zero);
      st(KIN_KW(link_quat) + 4 * l, T(0)); st(KIN_KW(link_quat) + 4 * l + 1, T(0)); st(KIN_KW(link_quat) + 4 * l + 2, T(0)); st(KIN_KW(link_quat) + 4 * l + 3, T(0));
    });
    if constexpr (!RB::SHOULDER) static_for<4>([&](auto ic) {
      constexpr int p = 20 + decltype(ic)::value;
      st3(KIN_KW(prim_point) + 3 * p, zero); st3(KIN_KW(prim_vel) + 3 * p, zero); st(KIN_KW(prim_force) + p, T(0));
    });
  }

  // leg L: its NJ moving links, the foot, and its knee, foot and (Solo12) shoulder primitives
  template <int L> SD void leg() {
    constexpr int L0 = 1 + L * (NJ + 1);
    const V3<T> zero = mk(T(0), T(0), T(0));
    // this leg's joints only (the arrays keep the whole robot's indexing, which leg_frames uses; the other entries are never read)
    T qd[NQ], sn[NQ], cs[NQ], sh[NQ], ch[NQ];
    static_for<NJ>([&](auto kc) {
      constexpr int j = RB::MD.links[L0 + decltype(kc)::value].dof;
      const T q = ld(STATE_SW(q) + j);
      qd[j] = ld(STATE_SW(qd) + j);
      const SinCos<T> full = sincos_call(q), half = sincos_call(q * T(0.5));
      sn[j] = full.s; cs[j] = full.c; sh[j] = half.s; ch[j] = half.c;
    });
    V3<T> kneeP, footP, shP = zero;
    leg_prim_points<T, ROBOT, L>(R0, sn, cs, kneeP, footP, shP);
    V3<T> op = zero, wp = w0, vop = v0;
    Quat<T> qp = Q0;
    leg_frames<T, ROBOT, L>(R0, sn, cs, [&](auto kc, const M3<T>& R, V3<T> o, V3<T> a) {
      constexpr int k = decltype(kc)::value;
      constexpr solorl_link_data LK = RB::MD.links[L0 + k];
      constexpr int AX = LK.axis[0] != 0.0 ? 0 : 1;
      static_assert(LK.parent == (k == 0 ? 0 : L0 + k - 1), "leg links are a chain from the base");
      const V3<T> w = fma3(a, qd[LK.dof], wp), vo = vop + cross(wp, o - op);
      const Quat<T> q = quat_rot_axis<AX>(qp, ch[LK.dof], sh[LK.dof]);
      link<L0 + k>(R, o, q, w, vo);
      if constexpr (RB::SHOULDER && k == 0) prim(20 + L, shP, o, w, vo);
      if constexpr (k == NJ - 2) prim(12 + 2 * L, kneeP, o, w, vo);
      if constexpr (k == NJ - 1) {       // the foot: a fixed child of the last link, with the leg's second primitive
        constexpr solorl_link_data FT = RB::MD.links[L0 + NJ];
        static_assert(FT.jtype == 1 && FT.parent == L0 + k, "foot link");
        const V3<T> of = addc(o, R, FT.jorigin[0], FT.jorigin[1], FT.jorigin[2]), vof = vo + cross(w, of - o);
        link<L0 + NJ>(R, of, q, w, vof);
        prim(13 + 2 * L, footP, of, w, vof);
      }
      op = o; wp = w; vop = vo; qp = q;
    });
  }

  // part 0 = base(), part 1 + L = leg<L>() (a compile-time part: the caller switches)
  template <int PART> SD void part() {
    if constexpr (PART == 0) base();
    else leg<PART - 1>();
  }
};

// the five shares, base first then the legs in order, and the totals' members of the output row
template <typename T, typename ST> SD void kin_totals(ST st, const KinSums<T> (&S)[KIN_PARTS]) {
  KinSums<T> A = S[0];
#pragma unroll
  for (int i = 1; i < KIN_PARTS; i++) {
    A.KE += S[i].KE; A.PE += S[i].PE; A.M += S[i].M;
    A.P = A.P + S[i].P; A.Lm = A.Lm + S[i].Lm; A.MC = A.MC + S[i].MC;
  }
  auto st3 = [&](int w, V3<T> v) { st(w, v.x); st(w + 1, v.y); st(w + 2, v.z); };
  const T iM = T(1) / A.M;
  st3(KIN_KW(com), A.MC * iM); st3(KIN_KW(com_vel), A.P * iM); st(KIN_KW(mass), A.M);
  st(KIN_KW(kinetic), A.KE); st(KIN_KW(potential), A.PE);
  st3(KIN_KW(lin_mom), A.P); st3(KIN_KW(ang_mom), A.Lm);
}

// the whole row by one caller
template <typename T, int ROBOT, typename LD, typename ST>
SD void env_kinematics(LD ld, ST st, int cmask, bool urdf, T sim_dt, T gravity) {
  KinSums<T> S[KIN_PARTS];
  static_for<KIN_PARTS>([&](auto pc) {
    KinRow<T, ROBOT, LD, ST> row(ld, st, cmask, urdf, sim_dt, gravity);
    row.template part<decltype(pc)::value>();
    S[decltype(pc)::value] = row.S;
  });
  kin_totals<T>(st, S);
}

// one row given as plain memory (the host program; any caller whose rows are not staged)
template <int ROBOT> SD void env_kinematics_row(const double* in, double* out, bool urdf, double sim_dt, double gravity) {
  int32_t cmask;
  __builtin_memcpy(&cmask, in + KIN_IN_MASK_WORD, sizeof(cmask));
  env_kinematics<double, ROBOT>([&](int w) { return in[w]; }, [&](int w, double v) { out[w] = v; }, cmask, urdf, sim_dt, gravity);
}

}  // namespace solo
