// nonfinite_main.cpp -- TEST ONLY.  Non-finite states through the kernel's sub-step code on the CPU (host_harness.cpp), as a
// stand-alone program so that it can be built with -fsanitize=address,undefined,float-cast-overflow and run as a child process
// (tests/test_host_nonfinite.py).  What it shows: the sub-step survives every poison the step kernels' NaN guard is documented to
// catch (include/solorl.h: "A per-env numeric failure (NaN/Inf state) is NOT an error") without a memory error or an undefined
// conversion, and the guard's sum (solorl_hip.hip, "A8 termination + NaN guard") is non-finite or beyond its 1e30 threshold
// whenever the state is.
//
//   nonfinite_main CONFIG...      each CONFIG: a file holding one solorl_config (the test writes the defaults of both robots)
// Built as it is it runs both robots in float and double; with -DHARNESS_ONLY_ROBOT=r -DHARNESS_ONLY_FLOAT=f one of the four (the test
// builds the four side by side: one translation unit with all of them takes the sanitizers several minutes).
//
// One line per (config, arithmetic type, treadmill, poison):
//   robot R T treadmill U poison NAME contacts 0xMASK state bad|ok guard fires|quiet
// Exit status 0 unless a robot failed to settle into contact or a file could not be read.
#include <cstdio>
#include <limits>
#include "host_harness.cpp"

namespace {
const double QNAN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();

struct Poison { const char* name; void (*apply)(solorl_env_state&); bool treadmill_only; };
const Poison POISONS[] = {
  {"action_nan", [](solorl_env_state& s) { s.tau[3] = QNAN; }, false},          // a NaN action survives the clip: the torque is NaN
  {"lin_vel_z_inf", [](solorl_env_state& s) { s.lin_vel[2] = INF; }, false},
  {"q_nan", [](solorl_env_state& s) { s.q[5] = QNAN; }, false},
  {"quat_x_nan", [](solorl_env_state& s) { s.quat[0] = QNAN; }, false},         // the guard sums qw only: must spread within the step
  {"pos_x_1e31", [](solorl_env_state& s) { s.pos[0] = 1e31; }, false},          // finite, above the guard's threshold
  {"pos_z_nan", [](solorl_env_state& s) { s.pos[2] = QNAN; }, false},
  {"pos_y_nan", [](solorl_env_state& s) { s.pos[1] = QNAN; }, true},            // the strip test |y - y_strip| <= half width
  {"ang_vel_neg_inf", [](solorl_env_state& s) { s.ang_vel[1] = -INF; }, false},
};

// the guard's condition, in the handle's arithmetic type and the kernel's order of summation
template <typename T> bool guard_fires(const solorl_env_state& s, int nq) {
  T chk = (T)s.pos[0] + (T)s.pos[1] + (T)s.pos[2] + (T)s.quat[3] + (T)s.lin_vel[0] + (T)s.lin_vel[1] + (T)s.lin_vel[2] + (T)s.ang_vel[0] +
          (T)s.ang_vel[1] + (T)s.ang_vel[2];
  for (int j = 0; j < nq; j++) chk += (T)s.q[j] + (T)s.qd[j];
  return !(std::fabs(chk) < T(1e30));
}

bool bad(double x) { return !(std::fabs(x) < 1e30); }
bool state_bad(const solorl_env_state& s, int nq) {
  bool b = false;
  for (int k = 0; k < 3; k++) b = b || bad(s.pos[k]) || bad(s.lin_vel[k]) || bad(s.ang_vel[k]);
  for (int k = 0; k < 4; k++) b = b || bad(s.quat[k]);
  for (int j = 0; j < nq; j++) b = b || bad(s.q[j]) || bad(s.qd[j]);
  return b;
}

// a crouched robot dropped from just above the ground, 240 zero-torque sub-steps (one second)
bool settled(const solorl_config& c, int use_float, solorl_env_state* out) {
  solorl_env_state s{};
  const int nq = c.robot == SOLORL_ROBOT_SOLO12 ? 12 : 8, per_leg = nq / 4;
  s.pos[2] = 0.3; s.quat[3] = 1.0;
  s.treadmill_y = c.use_treadmill ? c.treadmill_offset : 0.0;
  for (int leg = 0; leg < 4; leg++) {
    s.q[leg * per_leg + per_leg - 2] = 0.8;
    s.q[leg * per_leg + per_leg - 1] = -1.6;
  }
  for (int k = 0; k < 240; k++) harness_substep(&s, &c, use_float);
  *out = s;
  return (s.contact_mask & 0xFFFFFF) != 0 && !state_bad(s, nq);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s CONFIG...\n", argv[0]); return 2; }
  for (int a = 1; a < argc; a++) {
    solorl_config base;
    FILE* f = std::fopen(argv[a], "rb");
    if (!f || std::fread(&base, sizeof(base), 1, f) != 1) { std::fprintf(stderr, "cannot read a solorl_config from %s\n", argv[a]); return 2; }
    std::fclose(f);
    const int nq = base.robot == SOLORL_ROBOT_SOLO12 ? 12 : 8;
#ifdef HARNESS_ONLY_ROBOT                       // a build of one instantiation (host_harness.cpp): that robot and type only
    if (base.robot != HARNESS_ONLY_ROBOT) { std::fprintf(stderr, "%s: built for robot %d only\n", argv[a], HARNESS_ONLY_ROBOT); return 2; }
    for (int use_float = HARNESS_ONLY_FLOAT; use_float == HARNESS_ONLY_FLOAT; use_float = -1)
#else
    for (int use_float = 1; use_float >= 0; use_float--)
#endif
      for (int treadmill = 0; treadmill <= 1; treadmill++) {
        solorl_config c = base;
        c.use_treadmill = treadmill;
        solorl_env_state start;
        if (!settled(c, use_float, &start)) {
          std::fprintf(stderr, "robot %d %s treadmill %d: no contact after the settle\n", c.robot, use_float ? "float" : "double", treadmill);
          return 3;
        }
        for (const Poison& p : POISONS) {
          if (p.treadmill_only && !treadmill) continue;
          solorl_env_state s = start;
          p.apply(s);
          for (int ss = 0; ss < 4; ss++) harness_substep(&s, &c, use_float);      // (the harness clears tau after the first one: K8)
          const bool fires = use_float ? guard_fires<float>(s, nq) : guard_fires<double>(s, nq);
          std::printf("robot %d %s treadmill %d poison %s contacts 0x%x state %s guard %s\n", c.robot, use_float ? "float" : "double", treadmill,
                      p.name, (unsigned)start.contact_mask, state_bad(s, nq) ? "bad" : "ok", fires ? "fires" : "quiet");
        }
      }
  }
  return 0;
}
