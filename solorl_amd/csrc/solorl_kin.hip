// solorl_kinematics (include/solorl.h): link poses, support points of the collision primitives with their velocities and normal
// forces, centre of mass, energy and momentum of a batch of solorl_env_state rows, gfx950.  The arithmetic is csrc/kinematics.hpp
// (fp64), the memory shape around it csrc/row_batch.hpp (why rows are staged through LDS, a wavefront per leg); this file is that
// shape's numbers for this query, the order of the parts and the exchange of their shares, and the C entry point.
//
// A row in is 2040 B of which 74 words are read (the head pos .. lambda_prev, 73 contiguous words, and the contact_mask word), a row
// out is 3640 B.  A workgroup of four wavefronts takes KIN_ENVS consecutive rows; wavefront w runs leg w of every row, wavefront 0 the
// base with its twelve points before its leg (KinRow parts; the base is about a ninth of a leg's work).  LDS row strides are 148 and
// 910 dwords: of the eighteen lanes, rows 16 and 17 share banks with rows 0 and 1, the others fall on banks of their own.  The parts
// are independent up to their shares of the link sums, which all wavefronts leave where the staged input was (after a barrier);
// wavefront 0 adds the five in a fixed order and writes the totals (kin_totals).
// Residency, by both limits.  Registers: the kernel allocates 216 (Solo12) / 184 (Solo8) VGPRs, so a SIMD holds two wavefronts and a
// CU eight -- two workgroups of four.  LDS: a row costs (74 + 455) x 8 = 4232 B; KIN_ENVS = 18 rows are 76.2 KB of static LDS, two
// workgroups 152 KB of the CU's 160.  The two limits meet at two workgroups of 18 rows: 36 rows in flight per CU, one workgroup's
// copies beside the other's arithmetic.  (A fifth wavefront for the base, or more registers, would leave room for one workgroup only.)
// A row's arithmetic is a serial fp64 chain of ~9000 instructions, 24 calls of sincos_call among them.
#include <cmath>

#include "kinematics.hpp"
#include "row_batch.hpp"

namespace {

constexpr int KIN_ENVS = 18;        // envs per workgroup (solorl_amd/kinematics.py ENVS_PER_WORKGROUP says the same; tests/test_kin_static.py)
constexpr int KIN_WAVES = 4;        // wavefront w runs leg w of every row of the workgroup; wavefront 0 the base (a ninth of a leg's work) before it
using KinShell = solo::RowBatch<KIN_ENVS, solo::KIN_IN_WORDS, solo::KIN_OUT_WORDS, 64 * KIN_WAVES, 2>;
static_assert(KIN_WAVES + 1 == solo::KIN_PARTS, "four legs and the base");
static_assert(solo::KIN_PARTS * KIN_ENVS * solo::KIN_SUM_WORDS <= KIN_ENVS * solo::KIN_IN_WORDS, "the parts' sums take the staged input's place");

template <int ROBOT>
__global__ __launch_bounds__(64 * KIN_WAVES) void kin_rows_kernel(const double* __restrict__ states, const uint8_t* __restrict__ mask, int n,
                                                                   double* __restrict__ out, int urdf, double sim_dt, double gravity) {
  using namespace solo;
  __shared__ double s_in[KIN_ENVS * KIN_IN_WORDS];
  __shared__ double s_out[KIN_ENVS * KIN_OUT_WORDS];
  __shared__ int s_live[KIN_ENVS];
  const RowLane me = KinShell::rows_lane();
  KinShell::rows_live(s_live, mask, n);
  // (the staged row keeps the head's word offsets; the contact_mask word sits behind it: bits are copied, never converted)
  KinShell::rows_stage_in(s_in, s_live, states, [](int w) { return w < KIN_IN_HEAD_WORDS ? w : KIN_IN_MASK_WORD; });
  const bool mine = KinShell::rows_mine(s_live, me.lane);
  const double* in = s_in + me.lane * KIN_IN_WORDS;
  double* o = s_out + me.lane * KIN_OUT_WORDS;
  auto ld = [&](int w) { return in[w]; };
  auto st = [&](int w, double v) { o[w] = v; };
  using Row = KinRow<double, ROBOT, decltype(ld), decltype(st)>;
  KinSums<double> S{}, S0{};                               // this wavefront's leg; wavefront 0: the base as well
  if (mine) {
    int cmask;
    __builtin_memcpy(&cmask, in + KIN_IN_HEAD_WORDS, sizeof(cmask));
    if (me.wave == 0) {
      Row base(ld, st, cmask, urdf != 0, sim_dt, gravity);
      base.template part<0>();
      S0 = base.S;
    }
    Row row(ld, st, cmask, urdf != 0, sim_dt, gravity);
    run_leg_part(me.wave, row);
    S = row.S;
  }
  __syncthreads();                                         // every part has read what it needs of s_in: its place is free
  auto share = [&](int part) { return s_in + (part * KIN_ENVS + me.lane) * KIN_SUM_WORDS; };
  if (mine) {
    kin_sums_to_words(share(1 + me.wave), S);
    if (me.wave == 0) kin_sums_to_words(share(0), S0);
  }
  __syncthreads();
  if (me.wave == 0 && mine) {
    KinSums<double> P[KIN_PARTS];
#pragma unroll
    for (int k = 0; k < KIN_PARTS; k++) P[k] = kin_sums_from_words<double>(share(k));
    kin_totals<double>(st, P);
  }
  __syncthreads();
  KinShell::rows_stage_out(out, s_out, s_live);
}

}  // namespace

extern "C" int solorl_kinematics(const solorl_config* cfg, const solorl_env_state* states, const uint8_t* mask, int n, solorl_env_kin* out,
                                 int device_id, void* stream) {
  if (int rc = solo::rows_check_args("solorl_kinematics", cfg, states, out, n)) return rc;
  if (!(cfg->sim_dt > 0) || !std::isfinite(cfg->sim_dt)) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_kinematics: sim_dt must be > 0");
  if (!std::isfinite(cfg->gravity)) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_kinematics: gravity must be finite");
  if (int rc = solo::select_device(device_id)) return rc;
  return KinShell::launch("solorl_kinematics: kin_rows_kernel launch", cfg->robot == SOLORL_ROBOT_SOLO12 ? kin_rows_kernel<1> : kin_rows_kernel<0>, n, stream,
                          reinterpret_cast<const double*>(states), mask, n, reinterpret_cast<double*>(out), cfg->use_urdf_inertia, cfg->sim_dt, cfg->gravity);
}
