// dyn_tensors.hpp -- rigid-body dynamics tensors of ONE env's state row (include/solorl.h solorl_env_dyn): the joint-space mass matrix
// M(q), the bias force h(q, v) and its v = 0 part (gravity), and per foot the Jacobian of the lower leg's material point at the foot's
// support point, its Jdot v and the point itself.
//
// One function, env_dynamics<T, ROBOT>, made of five independent parts (the base and the four legs: DynRow) and the sum of their shares
// of the base's 6 x 6 block and of bias[0..5] (dyn_totals), the way kinematics.hpp is built.  solorl_dyn.hip runs a row's parts on four
// wavefronts, one lane per env each; tests/host/rows_main.cpp, compiled by g++ under SOLO_HOST_SHIM, calls the function as it is.  A row
// is read through `ld(word)` and written through `st(word, value)`; every word index is a compile-time constant after unrolling.
//
// Frames and support points are not restated: leg_frames and leg_prim_points of dynamics.hpp.  Everything is expressed as the step
// expresses it (spatial.hpp): world axes, origin at the base frame's origin `pos`, so the generalised velocity
// v = [lin_vel, ang_vel, qd] needs no transform and a joint's motion vector is S_j = (a_j, o_j x a_j).  What this file adds:
//   * per link the rigid-body inertia about pos (mass, first moment, rotational inertia: RBI) and, down a leg's chain, the composite
//     inertias I^c_k = sum of the links from joint k outwards;
//   * the columns of M from them, as in the composite-rigid-body algorithm: F = I^c_k S_k gives M[k][base] and M[k][j] = S_j . F
//     for the joints j between the base and k;
//   * one recursive Newton-Euler pass with all generalised accelerations zero: link velocities, bias accelerations
//     (alpha_k = alpha_p + qd_k w_p x a_k, a_o,k = a_o,p + alpha_p x r + w_p x (w_p x r)), the wrench each link needs
//     (m a_c + damping + weight, I alpha + w x I w + damping) taken about pos, summed outwards-in and projected on S_k: bias;
//   * the same with v = 0, which leaves the moments of the weights: gravity[k] = g (S_k.a x h^c_k)_z + g m^c_k (S_k.l)_z;
//   * the foot point P: columns e_k, e_k x P, a_j x (P - o_j) = a_j x P + S_j.l, and its bias acceleration from the lower leg's.
#pragma once
#include <cstddef>

#include "state_row.hpp"

namespace solo {

constexpr int DYN_NV = SOLORL_DYN_NV;                              // 18 = 6 + SOLORL_STATE_MAX_DOF
constexpr int DYN_OUT_WORDS = sizeof(solorl_env_dyn) / 8;          // 600
// the part of a state row that is read: pos .. qd, one contiguous segment
constexpr int DYN_IN_WORDS = (offsetof(solorl_env_state, qd) + sizeof(double) * SOLORL_STATE_MAX_DOF) / 8;   // 37
static_assert(sizeof(solorl_env_dyn) == 4800 && DYN_IN_WORDS == 37 && DYN_NV == 6 + SOLORL_STATE_MAX_DOF, "row sizes of include/solorl.h");
static_assert(offsetof(solorl_env_state, q) < offsetof(solorl_env_state, qd) && offsetof(solorl_env_state, ang_vel) < offsetof(solorl_env_state, q),
              "pos .. qd is the head of the state row");

#define DYN_DW(member) ((int)(offsetof(solorl_env_dyn, member) / 8))
#define DYN_M(a, b) (DYN_DW(mass_matrix) + (a) * DYN_NV + (b))
#define DYN_J(leg, r, c) (DYN_DW(foot_jac) + ((leg) * 3 + (r)) * DYN_NV + (c))

// a part's share of the whole robot's rigid-body inertia about pos (-> the base's 6 x 6 block, gravity[0..5]) and of the wrench
// about pos that the bias accelerations, the damping and the weights ask for (-> bias[0..5])
template <typename T> struct DynSums { RBI<T> I; SV<T> W; };
constexpr int DYN_SUM_WORDS = 16;
constexpr int DYN_PARTS = 5;          // the base, then one part per leg
// a share as DYN_SUM_WORDS words and back (how the device's wavefronts hand their shares to the one that adds them)
template <typename T> SD void dyn_sums_to_words(T* q, const DynSums<T>& A) {
  q[0] = A.I.m; q[1] = A.I.h.x; q[2] = A.I.h.y; q[3] = A.I.h.z;
  q[4] = A.I.I.xx; q[5] = A.I.I.xy; q[6] = A.I.I.xz; q[7] = A.I.I.yy; q[8] = A.I.I.yz; q[9] = A.I.I.zz;
  q[10] = A.W.a.x; q[11] = A.W.a.y; q[12] = A.W.a.z; q[13] = A.W.l.x; q[14] = A.W.l.y; q[15] = A.W.l.z;
}
template <typename T> SD DynSums<T> dyn_sums_from_words(const T* q) {
  return DynSums<T>{RBI<T>{q[0], mk(q[1], q[2], q[3]), Sym3<T>{q[4], q[5], q[6], q[7], q[8], q[9]}}, SV<T>{mk(q[10], q[11], q[12]), mk(q[13], q[14], q[15])}};
}

template <typename T> SD RBI<T> rbi_zero() { return RBI<T>{T(0), {T(0), T(0), T(0)}, {T(0), T(0), T(0), T(0), T(0), T(0)}}; }

// ld(w): word w of the state row (a member's STATE_SW offset + index);  st(w, v): word w of the solorl_env_dyn row.
// urdf: solorl_config use_urdf_inertia != 0;  gravity, kd: solorl_config gravity, damping.
template <typename T, int ROBOT, typename LD, typename ST> struct DynRow {
  using RB = Robot<ROBOT>;
  static constexpr int NJ = RB::NJ, NQ = RB::NQ, NL = RB::NL, NV = 6 + RB::NQ;
  LD ld; ST st;
  bool urdf; T gravity, kd;
  V3<T> pos, v0, w0; M3<T> R0;
  DynSums<T> S;

  SD DynRow(LD ld_, ST st_, bool urdf_, T gravity_, T kd_) : ld(ld_), st(st_), urdf(urdf_), gravity(gravity_), kd(kd_) {
    pos = mk(ld(STATE_SW(pos)), ld(STATE_SW(pos) + 1), ld(STATE_SW(pos) + 2));
    v0 = mk(ld(STATE_SW(lin_vel)), ld(STATE_SW(lin_vel) + 1), ld(STATE_SW(lin_vel) + 2));
    w0 = mk(ld(STATE_SW(ang_vel)), ld(STATE_SW(ang_vel) + 1), ld(STATE_SW(ang_vel) + 2));
    R0 = quat_to_mat(ld(STATE_SW(quat)), ld(STATE_SW(quat) + 1), ld(STATE_SW(quat) + 2), ld(STATE_SW(quat) + 3));   // the quaternion as it is, as the step reads it
    S = DynSums<T>{rbi_zero<T>(), zero6<T>()};
  }
  SD void st3(int w, V3<T> v) { st(w, v.x); st(w + 1, v.y); st(w + 2, v.z); }
  // M[a][b] and M[b][a] from one value
  SD void sym(int a, int b, T v) { st(DYN_M(a, b), v); if (a != b) st(DYN_M(b, a), v); }

  // whether generalised coordinate `col` is a joint of leg L
  template <int L> static constexpr bool own(int col) {
    for (int k = 0; k < NJ; k++) if (6 + RB::MD.links[1 + L * (NJ + 1) + k].dof == col) return true;
    return false;
  }

  // K2 inertia of link l about its COM, world axes: R I_l R^T (Bullet's box rule, or the URDF tensor)
  template <int l> SD Sym3<T> world_inertia(const M3<T>& R) const {
    const LinkInertia<T> I = link_inertia<T, ROBOT, l>(urdf);
    const V3<T> A0 = R.c0 * I.xx + R.c1 * I.xy + R.c2 * I.xz, A1 = R.c0 * I.xy + R.c1 * I.yy + R.c2 * I.yz, A2 = R.c0 * I.xz + R.c1 * I.yz + R.c2 * I.zz;
    return Sym3<T>{A0.x * R.c0.x + A1.x * R.c1.x + A2.x * R.c2.x, A0.x * R.c0.y + A1.x * R.c1.y + A2.x * R.c2.y,
                   A0.x * R.c0.z + A1.x * R.c1.z + A2.x * R.c2.z, A0.y * R.c0.y + A1.y * R.c1.y + A2.y * R.c2.y,
                   A0.y * R.c0.z + A1.y * R.c1.z + A2.y * R.c2.z, A0.z * R.c0.z + A1.z * R.c1.z + A2.z * R.c2.z};
  }

  // The mass of link l, riding on a body with axes R, a frame origin at o (relative to pos), angular velocity w, origin velocity vo and
  // bias accelerations alb (angular), aob (of the origin); rc = its COM relative to o.  add_wrench adds to W the wrench about pos it
  // needs at zero generalised accelerations, add_inertia its inertia about pos to I.
  template <int l> SD void add_wrench(const M3<T>& R, V3<T> o, V3<T> rc, V3<T> w, V3<T> vo, V3<T> alb, V3<T> aob, SV<T>& W) const {
    constexpr solorl_link_data LK = RB::MD.links[l];
    const T m = T(LK.mass);
    const V3<T> c = o + rc, wxrc = cross(w, rc);
    const V3<T> vc = vo + wxrc, acb = aob + cross(alb, rc) + cross(w, wxrc);
    const Sym3<T> Ic = world_inertia<l>(R);
    const V3<T> Iw = mul(Ic, w);
    // K3 damping: F = -m v_c (k + k |v_c|), T = -I w (k + k |w|)
    const T kl = kd + kd * sqrt_fast(dot(vc, vc)), ka = kd + kd * sqrt_fast(dot(w, w));
    V3<T> lin = fma3(vc, kl, acb) * m;
    lin.z += m * gravity;
    const V3<T> ang = mul(Ic, alb) + cross(w, Iw) + Iw * ka;
    W.l = W.l + lin;
    W.a = W.a + (ang + cross(c, lin));
  }
  template <int l> SD void add_inertia(const M3<T>& R, V3<T> c, RBI<T>& I) const {
    constexpr solorl_link_data LK = RB::MD.links[l];
    const T m = T(LK.mass);
    const Sym3<T> Ic = world_inertia<l>(R);
    const T cc = dot(c, c);
    I.m += m;
    I.h = fma3(c, m, I.h);
    I.I.xx += Ic.xx + m * (cc - c.x * c.x); I.I.xy += Ic.xy - m * c.x * c.y; I.I.xz += Ic.xz - m * c.x * c.z;
    I.I.yy += Ic.yy + m * (cc - c.y * c.y); I.I.yz += Ic.yz - m * c.y * c.z;
    I.I.zz += Ic.zz + m * (cc - c.z * c.z);
  }

  // the base link's share, and the coordinates a Solo8 does not have (they read 0 in every member the legs do not write)
  SD void base() {
    constexpr solorl_link_data LK = RB::MD.links[0];
    const V3<T> zero = mk(T(0), T(0), T(0));
    const V3<T> c = addc(zero, R0, LK.com[0], LK.com[1], LK.com[2]);
    add_wrench<0>(R0, zero, c, w0, v0, zero, zero, S.W);
    add_inertia<0>(R0, c, S.I);
    ROW_FENCE();
    static_for<DYN_NV - NV>([&](auto ic) {
      constexpr int a = NV + decltype(ic)::value;
      static_for<DYN_NV>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        st(DYN_M(a, b), T(0));
        if constexpr (b < 6) st(DYN_M(b, a), T(0));           // (rows 6 .. NV-1 of these columns: the legs, with their other-leg zeros)
      });
      st(DYN_DW(bias) + a, T(0)); st(DYN_DW(gravity) + a, T(0));
    });
  }

  // leg L: its joints' rows and columns of M, their bias and gravity entries, and foot L
  template <int L> SD void leg() {
    constexpr int L0 = 1 + L * (NJ + 1);
    const V3<T> zero = mk(T(0), T(0), T(0));
    // this leg's joints only (the arrays keep the whole robot's indexing, which leg_frames uses; the other entries are never read)
    T qd[NQ], sn[NQ], cs[NQ];
    static_for<NJ>([&](auto kc) {
      constexpr int j = RB::MD.links[L0 + decltype(kc)::value].dof;
      qd[j] = ld(STATE_SW(qd) + j);
      const SinCos<T> full = sincos_call(ld(STATE_SW(q) + j));
      sn[j] = full.s; cs[j] = full.c;
    });
    V3<T> kneeP, P, shP = zero;
    leg_prim_points<T, ROBOT, L>(R0, sn, cs, kneeP, P, shP);
    // the foot point and the columns of its Jacobian that belong to the base: 1 and e_k x P; the other legs' columns read 0
    st3(DYN_DW(foot_pos) + 3 * L, pos + P);
    static_for<3>([&](auto rc) {
      constexpr int r = decltype(rc)::value;
      static_for<3>([&](auto cc) { st(DYN_J(L, r, decltype(cc)::value), T(r == decltype(cc)::value ? 1 : 0)); });
      static_for<DYN_NV - 6>([&](auto cc) {
        constexpr int c = 6 + decltype(cc)::value;
        if constexpr (!own<L>(c)) st(DYN_J(L, r, c), T(0));
      });
    });
    st(DYN_J(L, 0, 3), T(0)); st(DYN_J(L, 0, 4), P.z);  st(DYN_J(L, 0, 5), -P.y);
    st(DYN_J(L, 1, 3), -P.z); st(DYN_J(L, 1, 4), T(0)); st(DYN_J(L, 1, 5), P.x);
    st(DYN_J(L, 2, 3), P.y);  st(DYN_J(L, 2, 4), -P.x); st(DYN_J(L, 2, 5), T(0));
    ROW_FENCE();

    // outwards: velocities, bias accelerations, each joint's motion vector and its column of the foot's Jacobian, each moving link's
    // inertia about pos and its wrench about pos -- the wrench projected at once on the motion vectors of the joints between the
    // base and the link (bias[j] = S_j . the wrenches from joint j outwards), so that only its sum is kept
    SV<T> Sj[NJ];
    RBI<T> Ik[NJ];
    T bj[NJ];
    V3<T> op = zero, wp = w0, vop = v0, albp = zero, aobp = zero;
    leg_frames<T, ROBOT, L>(R0, sn, cs, [&](auto kc, const M3<T>& R, V3<T> o, V3<T> a) {
      constexpr int k = decltype(kc)::value;
      constexpr solorl_link_data LK = RB::MD.links[L0 + k];
      static_assert(LK.parent == (k == 0 ? 0 : L0 + k - 1), "leg links are a chain from the base");
      const T qdk = qd[LK.dof];
      const V3<T> r = o - op, wxr = cross(wp, r);
      const V3<T> w = fma3(a, qdk, wp), vo = vop + wxr;
      const V3<T> alb = fma3(cross(wp, a), qdk, albp), aob = aobp + cross(albp, r) + cross(wp, wxr);
      Sj[k] = SV<T>{a, cross(o, a)};
      const V3<T> jc = cross(a, P) + Sj[k].l;                    // a x (P - o)
      st(DYN_J(L, 0, 6 + LK.dof), jc.x); st(DYN_J(L, 1, 6 + LK.dof), jc.y); st(DYN_J(L, 2, 6 + LK.dof), jc.z);
      SV<T> W = zero6<T>();
      Ik[k] = rbi_zero<T>();
      const V3<T> rc = addc(zero, R, LK.com[0], LK.com[1], LK.com[2]);
      add_wrench<L0 + k>(R, o, rc, w, vo, alb, aob, W);
      add_inertia<L0 + k>(R, o + rc, Ik[k]);
      if constexpr (k == NJ - 1) {       // the foot: a fixed child of the last link, a second mass on the same body
        constexpr solorl_link_data FT = RB::MD.links[L0 + NJ];
        static_assert(FT.jtype == 1 && FT.parent == L0 + k, "foot link");
        const V3<T> rf = addc(addc(zero, R, FT.jorigin[0], FT.jorigin[1], FT.jorigin[2]), R, FT.com[0], FT.com[1], FT.com[2]);
        add_wrench<L0 + NJ>(R, o, rf, w, vo, alb, aob, W);
        add_inertia<L0 + NJ>(R, o + rf, Ik[k]);
        // Jdot v: the material point's acceleration at zero generalised accelerations
        const V3<T> rp = P - o;
        st3(DYN_DW(foot_acc_bias) + 3 * L, aob + cross(alb, rp) + cross(w, cross(w, rp)));
      }
      static_for<k + 1>([&](auto jc_) {
        constexpr int j = decltype(jc_)::value;
        if constexpr (j == k) bj[j] = dot(Sj[j], W);
        else bj[j] += dot(Sj[j], W);
      });
      S.W = S.W + W;
      op = o; wp = w; vop = vo; albp = alb; aobp = aob;
      ROW_FENCE();
    });
    static_for<NJ>([&](auto kc) { st(DYN_DW(bias) + 6 + RB::MD.links[L0 + decltype(kc)::value].dof, bj[decltype(kc)::value]); });

    // inwards: the composite inertia from joint k outwards, row 6 + dof_k of M, gravity
    static_for<NJ>([&](auto ic) {
      constexpr int k = NJ - 1 - decltype(ic)::value;
      constexpr int row = 6 + RB::MD.links[L0 + k].dof;
      add(S.I, Ik[k]);
      const SV<T> F = mul(S.I, Sj[k]);                          // (a: moment about pos, l: force) of a unit rate of joint k
      sym(row, 0, F.l.x); sym(row, 1, F.l.y); sym(row, 2, F.l.z);
      sym(row, 3, F.a.x); sym(row, 4, F.a.y); sym(row, 5, F.a.z);
      static_for<k + 1>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        sym(row, 6 + RB::MD.links[L0 + j].dof, dot(Sj[j], F));
      });
      static_for<DYN_NV - 6>([&](auto cc) {                     // no coupling with the other legs' joints
        constexpr int c = 6 + decltype(cc)::value;
        if constexpr (!own<L>(c)) st(DYN_M(row, c), T(0));
      });
      st(DYN_DW(gravity) + row, gravity * (Sj[k].a.x * S.I.h.y - Sj[k].a.y * S.I.h.x + Sj[k].l.z * S.I.m));
      ROW_FENCE();
    });
  }

  // part 0 = base(), part 1 + L = leg<L>() (a compile-time part: the caller switches)
  template <int PART> SD void part() {
    if constexpr (PART == 0) base();
    else leg<PART - 1>();
  }
};

// A += B, member by member (the order in which the shares are added is the caller's: base first, then the legs in order)
template <typename T> SD void dyn_add(DynSums<T>& A, const DynSums<T>& B) { add(A.I, B.I); A.W = A.W + B.W; }

// the whole robot's inertia and wrench about pos -> the base's 6 x 6 block of M, bias[0..5], gravity[0..5]
//   [lin; ang] block of a rigid body about pos:  [[m 1, -[h]x], [[h]x, I]]
template <typename T, typename ST> SD void dyn_totals(ST st, const DynSums<T>& A, T gravity) {
  auto sym = [&](int a, int b, T v) { st(DYN_M(a, b), v); if (a != b) st(DYN_M(b, a), v); };
  const RBI<T>& I = A.I;
  sym(0, 0, I.m); sym(1, 1, I.m); sym(2, 2, I.m);
  sym(0, 1, T(0)); sym(0, 2, T(0)); sym(1, 2, T(0));
  sym(0, 3, T(0)); sym(0, 4, I.h.z); sym(0, 5, -I.h.y);
  sym(1, 3, -I.h.z); sym(1, 4, T(0)); sym(1, 5, I.h.x);
  sym(2, 3, I.h.y); sym(2, 4, -I.h.x); sym(2, 5, T(0));
  sym(3, 3, I.I.xx); sym(3, 4, I.I.xy); sym(3, 5, I.I.xz); sym(4, 4, I.I.yy); sym(4, 5, I.I.yz); sym(5, 5, I.I.zz);
  st(DYN_DW(bias) + 0, A.W.l.x); st(DYN_DW(bias) + 1, A.W.l.y); st(DYN_DW(bias) + 2, A.W.l.z);
  st(DYN_DW(bias) + 3, A.W.a.x); st(DYN_DW(bias) + 4, A.W.a.y); st(DYN_DW(bias) + 5, A.W.a.z);
  // the weight (0, 0, m g) and its moment about pos, h x (0, 0, g)
  st(DYN_DW(gravity) + 0, T(0)); st(DYN_DW(gravity) + 1, T(0)); st(DYN_DW(gravity) + 2, I.m * gravity);
  st(DYN_DW(gravity) + 3, I.h.y * gravity); st(DYN_DW(gravity) + 4, -(I.h.x * gravity)); st(DYN_DW(gravity) + 5, T(0));
}

// the whole row by one caller
template <typename T, int ROBOT, typename LD, typename ST>
SD void env_dynamics(LD ld, ST st, bool urdf, T gravity, T kd) {
  DynSums<T> A;
  static_for<DYN_PARTS>([&](auto pc) {
    DynRow<T, ROBOT, LD, ST> row(ld, st, urdf, gravity, kd);
    row.template part<decltype(pc)::value>();
    if constexpr (decltype(pc)::value == 0) A = row.S;
    else dyn_add(A, row.S);
  });
  dyn_totals<T>(st, A, gravity);
}

// one row given as plain memory (the host program; any caller whose rows are not staged)
template <int ROBOT> SD void env_dynamics_row(const double* in, double* out, bool urdf, double gravity, double kd) {
  env_dynamics<double, ROBOT>([&](int w) { return in[w]; }, [&](int w, double v) { out[w] = v; }, urdf, gravity, kd);
}

}  // namespace solo
