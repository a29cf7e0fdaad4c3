// solorl_dynamics (include/solorl.h): joint-space mass matrix, bias and gravity forces, foot Jacobians with their Jdot v and foot points
// of a batch of solorl_env_state rows, gfx950.  The arithmetic is csrc/dyn_tensors.hpp (fp64), the memory shape around it
// csrc/row_batch.hpp (why rows are staged through LDS, a wavefront per leg); this file is that shape's numbers for this query, the order
// of the parts and the exchange of their shares, and the C entry point.
//
// A row in is 2040 B of which the 37 contiguous words pos .. qd are read, a row out is 4800 B, and the 324 words of M do not fit a
// lane's registers: every output word is stored to LDS as soon as it exists.  A workgroup of four wavefronts takes DYN_ENVS consecutive
// rows; wavefront w runs leg w of every row, wavefront 0 the base link after its leg (DynRow parts).  The parts are independent up to
// their shares of the robot's inertia and wrench about pos (16 words each): behind a barrier the staged input's place (37 words per
// row) takes the shares of legs 1 and 2, wavefront 0 adds them to its own (base, leg 0, leg 1, leg 2: the order of env_dynamics), then
// it takes leg 3's share the same way, and wavefront 0 writes the base's 6 x 6 block, bias[0..5] and gravity[0..5] (dyn_totals).
// Residency.  LDS: a row costs (37 + 600) x 8 = 5096 B; DYN_ENVS = 16 rows and their live flags are 81 600 B of static LDS, two
// workgroups 163 200 B of the CU's 163 840.  Registers: the kernel allocates 248 (Solo12) / 224 (Solo8) VGPRs and no AGPRs, so a SIMD
// holds two wavefronts and a CU eight -- two workgroups of four, by both limits: one workgroup's copies beside the other's arithmetic.
#include <cmath>

#include "dyn_tensors.hpp"
#include "row_batch.hpp"

namespace {

constexpr int DYN_ENVS = 16;        // envs per workgroup (solorl_amd/dyn_tensors.py ENVS_PER_WORKGROUP says the same; tests/test_dyn_static.py)
constexpr int DYN_WAVES = 4;        // wavefront w runs leg w of every row of the workgroup; wavefront 0 the base link after it
using DynShell = solo::RowBatch<DYN_ENVS, solo::DYN_IN_WORDS, solo::DYN_OUT_WORDS, 64 * DYN_WAVES, 1>;
static_assert(DYN_WAVES + 1 == solo::DYN_PARTS, "four legs and the base");
static_assert(2 * solo::DYN_SUM_WORDS <= solo::DYN_IN_WORDS, "two parts' shares at a time take the staged input's place");

template <int ROBOT>
__global__ __launch_bounds__(64 * DYN_WAVES) void dyn_rows_kernel(const double* __restrict__ states, const uint8_t* __restrict__ mask, int n,
                                                                   double* __restrict__ out, int urdf, double gravity, double damping) {
  using namespace solo;
  __shared__ double s_in[DYN_ENVS * DYN_IN_WORDS];
  __shared__ double s_out[DYN_ENVS * DYN_OUT_WORDS];
  __shared__ int s_live[DYN_ENVS];
  const RowLane me = DynShell::rows_lane();
  DynShell::rows_live(s_live, mask, n);
  DynShell::rows_stage_in(s_in, s_live, states, [](int w) { return w; });
  const bool mine = DynShell::rows_mine(s_live, me.lane);
  const double* in = s_in + me.lane * DYN_IN_WORDS;
  double* o = s_out + me.lane * DYN_OUT_WORDS;
  auto ld = [&](int w) { return in[w]; };
  auto st = [&](int w, double v) { o[w] = v; };
  using Row = DynRow<double, ROBOT, decltype(ld), decltype(st)>;
  DynSums<double> S{};                                     // this wavefront's leg; wavefront 0: the base plus its leg
  if (mine) {
    Row row(ld, st, urdf != 0, gravity, damping);
    run_leg_part(me.wave, row);
    S = row.S;
    if (me.wave == 0) {                                    // (after its leg, so that the base's share is not held through it)
      Row base(ld, st, urdf != 0, gravity, damping);
      base.template part<0>();
      dyn_add(base.S, S);
      S = base.S;
    }
  }
  __syncthreads();                                         // every part has read what it needs of s_in: its place is free
  double* slot = s_in + me.lane * DYN_IN_WORDS;            // this row's two slots of DYN_SUM_WORDS
  auto put = [&](int k, const DynSums<double>& A) { dyn_sums_to_words(slot + k * DYN_SUM_WORDS, A); };
  auto take = [&](int k) { return dyn_sums_from_words<double>(slot + k * DYN_SUM_WORDS); };
  if (mine && (me.wave == 1 || me.wave == 2)) put(me.wave - 1, S);
  __syncthreads();
  if (mine && me.wave == 0) { dyn_add(S, take(0)); dyn_add(S, take(1)); }
  __syncthreads();
  if (mine && me.wave == 3) put(0, S);
  __syncthreads();
  if (mine && me.wave == 0) {
    dyn_add(S, take(0));
    dyn_totals<double>(st, S, gravity);
  }
  __syncthreads();
  DynShell::rows_stage_out(out, s_out, s_live);
}

}  // namespace

extern "C" int solorl_dynamics(const solorl_config* cfg, const solorl_env_state* states, const uint8_t* mask, int n, solorl_env_dyn* out,
                               int device_id, void* stream) {
  if (int rc = solo::rows_check_args("solorl_dynamics", cfg, states, out, n)) return rc;
  if (!std::isfinite(cfg->gravity)) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_dynamics: gravity must be finite");
  if (!std::isfinite(cfg->damping) || cfg->damping < 0) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_dynamics: damping must be finite and >= 0");
  if (int rc = solo::select_device(device_id)) return rc;
  return DynShell::launch("solorl_dynamics: dyn_rows_kernel launch", cfg->robot == SOLORL_ROBOT_SOLO12 ? dyn_rows_kernel<1> : dyn_rows_kernel<0>, n, stream,
                          reinterpret_cast<const double*>(states), mask, n, reinterpret_cast<double*>(out), cfg->use_urdf_inertia, cfg->gravity, cfg->damping);
}
