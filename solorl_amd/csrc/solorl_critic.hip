// solorl_critic_obs (include/solorl.h, "Privileged critic rows"): the critic's row of a batch of solorl_env_state rows -- the clean
// observation row and twenty words of the simulator's truth behind it -- gfx950.  The arithmetic is csrc/critic_obs.hpp (fp64), the
// memory shape around it csrc/row_batch.hpp (why rows are staged through LDS, a wavefront per leg); this file is that shape's numbers
// for this query, the order of the phases, and the C entry point.
//
// A row in is 2040 B of which 55 words are read (what the shaped terms read -- pos .. tau, lambda_prev of the four foot primitives,
// the contact_mask word -- and the timestep word), E floats of obs_in, and of the env's command, actuator and kick rows 3 doubles,
// 13 words and 2 doubles; a row out is E + 20 floats.  A workgroup of four wavefronts takes CRITIC_ENVS consecutive rows; wavefront w
// runs leg w of every row (a KinRow whose store keeps the foot's seven words and nothing else) and leaves them in LDS; behind a barrier
// wavefront 0 turns every row's feet, counters and the env's three small rows (read by the row's lane straight from global memory: at
// most 100 B per row, not staged) into the twenty words, as floats in LDS; behind a second barrier all lanes copy the workgroup's
// piece of obs_in, consecutive lanes on consecutive words of it, into the rows of critic_out, and then the twenty words out of LDS
// behind them.  The walk along obs_in needs one division per thread, by the host, none in the loop.
// One LDS row holds 55 + 28 = 83 words.  83 is odd, so the 64 lanes' 8-byte accesses at one immediate offset fall on 64 different
// bank pairs: no conflict in the arithmetic.
// Residency, by both limits.  LDS: 83 x 8 B + the live flag + 20 floats = 748 B per row, 47 872 B of static LDS at CRITIC_ENVS = 64 (the
// lanes of a wavefront bound the rows, not the LDS): three workgroups per CU would fit (143.6 KB of 160).  Registers (the compiler's
// resource remarks): 100 VGPRs (Solo12) / 98 (Solo8), 80 SGPRs, no AGPRs, no scratch -- the legs are the shaped terms' -- which would
// let four waves share a SIMD: LDS decides, three workgroups of 64 rows per CU (the remarks' occupancy: 3 waves per SIMD), one
// workgroup's copies beside another's arithmetic.
#include <cmath>

#include "critic_obs.hpp"
#include "row_batch.hpp"

namespace {

constexpr int CRITIC_ENVS = 64;     // envs per workgroup: every lane of a wavefront has a row (solorl_amd/critic_obs.py ENVS_PER_WORKGROUP says the same)
constexpr int CRITIC_WAVES = 4;     // wavefront w runs leg w of every row of the workgroup; wavefront 0 the twenty words after it
constexpr int CRITIC_THREADS = 64 * CRITIC_WAVES;
constexpr int CRITIC_OFF_FEET = solo::CRITIC_IN_WORDS;
constexpr int CRITIC_ROW_WORDS = CRITIC_OFF_FEET + solo::SHAPE_FEET_WORDS;     // 83
using CriticShell = solo::RowBatch<CRITIC_ENVS, solo::CRITIC_IN_WORDS, solo::SHAPE_FEET_WORDS, CRITIC_THREADS, 2>;
static_assert(CRITIC_ROW_WORDS == 83 && CRITIC_ROW_WORDS % 2 == 1, "an odd row stride: lane = row accesses at one offset are conflict-free");
static_assert(CriticShell::LDS_BYTES == (size_t)CRITIC_ENVS * (CRITIC_ROW_WORDS * 8 + 4), "static LDS of the kernel but for the twenty words");
// the kernel's whole static LDS (the shell's rows and live flags, and the twenty words as floats): what the residency above is counted from
constexpr size_t CRITIC_LDS_BYTES = CriticShell::LDS_BYTES + (size_t)CRITIC_ENVS * solo::CRITIC_PRIV * sizeof(float);
static_assert(CRITIC_LDS_BYTES == 47872 && 3 * CRITIC_LDS_BYTES <= 160 * 1024, "three workgroups share the LDS of a CU");

// dr, dc = CRITIC_THREADS / E, CRITIC_THREADS % E: the (rows, words) between a thread's consecutive observation words
template <int ROBOT>
__global__ __launch_bounds__(CRITIC_THREADS) void critic_rows_kernel(const double* __restrict__ states, const uint8_t* __restrict__ mask, int n, int E, int dr,
                                                                     int dc, const float* __restrict__ obs_in, const solorl_env_command* __restrict__ cmd,
                                                                     const solorl_env_actuator* __restrict__ act, const double* __restrict__ kick,
                                                                     float* __restrict__ out, solo::CriticScale S, double sim_dt) {
  using namespace solo;
  __shared__ double s_row[CRITIC_ENVS * CRITIC_ROW_WORDS];
  __shared__ float s_priv[CRITIC_ENVS * CRITIC_PRIV];
  __shared__ int s_live[CRITIC_ENVS];
  static_assert(sizeof(s_row) + sizeof(s_priv) + sizeof(s_live) == CRITIC_LDS_BYTES, "the kernel's static LDS");
  const RowLane me = CriticShell::rows_lane();
  CriticShell::rows_live(s_live, mask, n);
#pragma unroll 2
  for (int idx = threadIdx.x; idx < CRITIC_ENVS * CRITIC_IN_WORDS; idx += CRITIC_THREADS) {
    const int r = idx / CRITIC_IN_WORDS, w = idx - r * CRITIC_IN_WORDS;
    if (s_live[r]) s_row[r * CRITIC_ROW_WORDS + w] = states[(size_t)(CriticShell::first_row() + r) * STATE_WORDS + critic_in_word(w)];
  }
  __syncthreads();
  const bool mine = CriticShell::rows_mine(s_live, me.lane);
  double* row = s_row + me.lane * CRITIC_ROW_WORDS;
  auto ld = [&](int w) { return row[shape_staged_word(w)]; };
  int cmask = 0;
  if (mine) {
    __builtin_memcpy(&cmask, row + SHAPE_IN_WORDS - 1, sizeof(cmask));
    auto st = shape_foot_store([&](int k, double v) { row[CRITIC_OFF_FEET + k] = v; });
    KinRow<double, ROBOT, decltype(ld), decltype(st)> leg(ld, st, cmask, false, sim_dt, 0.0);
    run_leg_part(me.wave, leg);
  }
  __syncthreads();                                         // the four feet of every row are in LDS
  if (me.wave == 0 && mine) {
    const size_t i = (size_t)CriticShell::first_row() + me.lane;
    int timestep;
    __builtin_memcpy(&timestep, row + CRITIC_IN_TIME, sizeof(timestep));
    critic_priv<ROBOT>([&](int k) { return row[CRITIC_OFF_FEET + k]; }, cmask, timestep, cmd ? cmd[i].cmd : nullptr, act ? act + i : nullptr,
                       kick ? kick + i * 6 : nullptr, S, [&](int k, float v) { s_priv[me.lane * CRITIC_PRIV + k] = v; });
  }
  __syncthreads();                                         // the twenty words of every row are in LDS
  const int O = E + CRITIC_PRIV, first = CriticShell::first_row();
  const int rows = n - first < CRITIC_ENVS ? n - first : CRITIC_ENVS;
  const float* in = obs_in + (size_t)first * E;
  float* dst = out + (size_t)first * O;
  // the observation words: consecutive lanes on consecutive words of obs_in, which is ONE contiguous piece (masked rows' words skipped)
  int r = (int)threadIdx.x / E, c = (int)threadIdx.x - r * E;
#pragma unroll 2
  for (int idx = threadIdx.x; idx < rows * E; idx += CRITIC_THREADS) {
    if (s_live[r]) dst[(size_t)r * O + c] = in[idx];
    r += dr;
    c += dc;
    if (c >= E) { c -= E; r++; }
  }
  // the twenty words behind them, from LDS (a loop of its own: one loop whose word comes from either memory reads both through FLAT)
  for (int idx = threadIdx.x; idx < rows * CRITIC_PRIV; idx += CRITIC_THREADS) {
    const int pr = idx / CRITIC_PRIV, k = idx - pr * CRITIC_PRIV;
    if (s_live[pr]) dst[(size_t)pr * O + E + k] = s_priv[idx];
  }
}

}  // namespace

extern "C" int solorl_critic_obs(const solorl_config* cfg, const solorl_critic_params* p, const solorl_env_state* states, const uint8_t* mask, int n,
                                 const float* obs_in, const solorl_env_command* cmd, const solorl_env_actuator* act, const double* kick, float* critic_out,
                                 int device_id, void* stream) {
  const char* fn = "solorl_critic_obs";
  if (int rc = solo::rows_check_args(fn, cfg, states, critic_out, n)) return rc;
  if (!p || !obs_in) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_critic_obs: null params or obs_in");
  if (p->obs_dim < 1 || p->obs_dim > solo::CRITIC_MAX_OBS) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_critic_obs: obs_dim must be 1..210");
  solo::CriticScale S;
  for (int k = 0; k < solo::CRITIC_PRIV; k++) {
    if (!std::isfinite(p->scale[k])) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_critic_obs: every scale must be finite");
    S.s[k] = p->scale[k];
  }
  if (int rc = solo::select_device(device_id)) return rc;
  return CriticShell::launch("solorl_critic_obs: critic_rows_kernel launch", cfg->robot == SOLORL_ROBOT_SOLO12 ? critic_rows_kernel<1> : critic_rows_kernel<0>, n,
                             stream, reinterpret_cast<const double*>(states), mask, n, p->obs_dim, CRITIC_THREADS / p->obs_dim, CRITIC_THREADS % p->obs_dim, obs_in, cmd, act, kick,
                             critic_out, S, cfg->sim_dt);
}
