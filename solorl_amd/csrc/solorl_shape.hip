// solorl_shape_reward (include/solorl.h): sixteen shaped reward terms of a batch of solorl_env_state rows, added to the step's reward,
// with the per-env memory they need (solorl_env_shape rows), gfx950.  The arithmetic is csrc/reward_shape.hpp (fp64), the memory shape
// around it csrc/row_batch.hpp (why rows are staged through LDS, a wavefront per leg); this file is that shape's numbers for this query,
// the order of the phases, and the C entry point.
//
// A row in is 2040 B of which 54 words are read (pos .. tau, 49 contiguous words, lambda_prev of the four foot primitives and the
// contact_mask word) plus the env's 45-word memory row; a row out is that memory row and, if asked for, 16 term values.  A workgroup of
// four wavefronts takes SHAPE_ENVS consecutive rows; wavefront w runs leg w of every row (a KinRow whose store keeps the foot's seven
// words and nothing else) and leaves them in LDS; behind a barrier wavefront 0 evaluates the terms of every row, rewrites the staged
// memory row in place and touches actions, done, reward and ep_out -- one small typed access per lane and value, the owning lane's
// (ep_out is field-major: consecutive lanes, consecutive addresses).  All lanes copy the memory rows and the terms out.
// One LDS row holds everything of an env: 54 + 45 + 28 + 16 = 143 words.  143 is odd, so the 64 lanes' 8-byte accesses at one immediate
// offset fall on 64 different bank pairs: no conflict in any phase of the arithmetic.
// solorl_shape_reward_cmd: the tracking terms' command is the row's own (a solorl_env_command row's three doubles, read by the lane that
// evaluates the row's terms straight from global memory: 24 B per row, not staged); solorl_shape_reward is that call without rows.
// Residency, by both limits.  LDS: 143 x 8 B + the live flag = 1148 B per row; two workgroups per CU may hold 80 KB each, 71 rows -- more
// than the 64 lanes of a wavefront, so the lanes bound it: SHAPE_ENVS = 64, 73 472 B of static LDS, two workgroups 143.5 KB of the CU's
// 160 (a third would need 215).  Registers: a leg is KinRow's chain without its stores and sums, 100 VGPRs (Solo12) / 98 (Solo8), no
// AGPRs, no scratch: four workgroups would fit by registers, so LDS decides.  Two workgroups of 64 rows per CU: 128 rows in flight,
// every lane busy, one workgroup's copies beside the other's arithmetic.
#include <cmath>

#include "reward_shape.hpp"
#include "row_batch.hpp"

namespace {

constexpr int SHAPE_ENVS = 64;      // envs per workgroup: every lane of a wavefront has a row (solorl_amd/shaping.py ENVS_PER_WORKGROUP says the same)
constexpr int SHAPE_WAVES = 4;      // wavefront w runs leg w of every row of the workgroup; wavefront 0 the terms after it
// one env's LDS row: staged state words, memory row, the feet's words, the terms
constexpr int SHAPE_OFF_MEM = solo::SHAPE_IN_WORDS, SHAPE_OFF_FEET = SHAPE_OFF_MEM + solo::SHAPE_MEM_WORDS, SHAPE_OFF_TERMS = SHAPE_OFF_FEET + solo::SHAPE_FEET_WORDS;
constexpr int SHAPE_ROW_WORDS = SHAPE_OFF_TERMS + solo::SHAPE_TERMS;     // 143
using ShapeShell = solo::RowBatch<SHAPE_ENVS, solo::SHAPE_IN_WORDS, SHAPE_ROW_WORDS - solo::SHAPE_IN_WORDS, 64 * SHAPE_WAVES, 2>;
static_assert(SHAPE_ROW_WORDS == 143 && SHAPE_ROW_WORDS % 2 == 1, "an odd row stride: lane = row accesses at one offset are conflict-free");
static_assert(ShapeShell::LDS_BYTES == (size_t)SHAPE_ENVS * (SHAPE_ROW_WORDS * 8 + 4), "static LDS of the kernel");

// WORDS words of every live row between global memory and the rows' LDS section at `off`, lane after lane along each row
// src(row, w): the value of word w of global row `row`
template <int WORDS, typename SRC> __device__ __forceinline__ void rows_copy_in(double* s_row, int off, const int* s_live, SRC src) {
#pragma unroll 2
  for (int idx = threadIdx.x; idx < SHAPE_ENVS * WORDS; idx += 64 * SHAPE_WAVES) {
    const int r = idx / WORDS, w = idx - r * WORDS;
    if (s_live[r]) s_row[r * SHAPE_ROW_WORDS + off + w] = src((size_t)(ShapeShell::first_row() + r), w);
  }
}
template <int WORDS> __device__ __forceinline__ void rows_copy_out(double* dst, const double* s_row, int off, const int* s_live) {
  dst += (size_t)ShapeShell::first_row() * WORDS;
#pragma unroll 2
  for (int idx = threadIdx.x; idx < SHAPE_ENVS * WORDS; idx += 64 * SHAPE_WAVES) {
    const int r = idx / WORDS, w = idx - r * WORDS;
    if (s_live[r]) dst[idx] = s_row[r * SHAPE_ROW_WORDS + off + w];
  }
}

template <int ROBOT>
__global__ __launch_bounds__(64 * SHAPE_WAVES) void shape_rows_kernel(const double* __restrict__ states, const uint8_t* __restrict__ mask, int n,
                                                                       const float* __restrict__ actions, const uint8_t* __restrict__ done,
                                                                       double* __restrict__ mem, float* __restrict__ reward, double* __restrict__ terms_out,
                                                                       double* __restrict__ ep_out, const solorl_env_command* __restrict__ cmd,
                                                                       solorl_shape_params P, double sim_dt, double dtc) {
  using namespace solo;
  __shared__ double s_row[SHAPE_ENVS * SHAPE_ROW_WORDS];
  __shared__ int s_live[SHAPE_ENVS];
  const RowLane me = ShapeShell::rows_lane();
  ShapeShell::rows_live(s_live, mask, n);
  rows_copy_in<SHAPE_IN_WORDS>(s_row, 0, s_live, [&](size_t row, int w) { return states[row * STATE_WORDS + shape_in_word(w)]; });
  rows_copy_in<SHAPE_MEM_WORDS>(s_row, SHAPE_OFF_MEM, s_live, [&](size_t row, int w) { return mem[row * SHAPE_MEM_WORDS + w]; });
  __syncthreads();
  const bool mine = ShapeShell::rows_mine(s_live, me.lane);
  double* row = s_row + me.lane * SHAPE_ROW_WORDS;
  auto ld = [&](int w) { return row[shape_staged_word(w)]; };
  int cmask = 0;
  if (mine) {
    __builtin_memcpy(&cmask, row + SHAPE_IN_WORDS - 1, sizeof(cmask));
    auto st = shape_foot_store([&](int k, double v) { row[SHAPE_OFF_FEET + k] = v; });
    KinRow<double, ROBOT, decltype(ld), decltype(st)> leg(ld, st, cmask, false, sim_dt, 0.0);
    run_leg_part(me.wave, leg);
  }
  __syncthreads();                                         // the four feet of every row are in LDS
  if (me.wave == 0 && mine) {
    const size_t i = (size_t)ShapeShell::first_row() + me.lane;
    shape_row<ROBOT>(ld, cmask, [&](int k) { return row[SHAPE_OFF_FEET + k]; }, [&](int w) { return row[SHAPE_OFF_MEM + w]; },
                     [&](int w, double v) { row[SHAPE_OFF_MEM + w] = v; }, [&](int k, double v) { row[SHAPE_OFF_TERMS + k] = v; },
                     [&](int k, double v) { if (ep_out) ep_out[(size_t)k * n + i] += v; }, P, sim_dt, dtc,
                     actions + i * Robot<ROBOT>::NQ, done != nullptr && done[i] != 0, reward ? reward + i : nullptr, cmd ? cmd[i].cmd : nullptr);
  }
  __syncthreads();
  rows_copy_out<SHAPE_MEM_WORDS>(mem, s_row, SHAPE_OFF_MEM, s_live);
  if (terms_out) rows_copy_out<SHAPE_TERMS>(terms_out, s_row, SHAPE_OFF_TERMS, s_live);
}

}  // namespace

extern "C" int solorl_shape_reward_cmd(const solorl_config* cfg, const solorl_shape_params* p, const solorl_env_state* states, const uint8_t* mask, int n,
                                       const float* actions, const uint8_t* done, solorl_env_shape* mem, float* reward, double* terms_out, double* ep_out,
                                       const solorl_env_command* cmd, int device_id, void* stream) {
  const char* fn = "solorl_shape_reward";
  if (int rc = solo::rows_check_args(fn, cfg, states, mem, n)) return rc;
  if (!p || !actions) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_shape_reward: null params or actions");
  bool finite = true;
  for (size_t k = 0; k < sizeof(*p) / sizeof(double); k++) finite = finite && std::isfinite(reinterpret_cast<const double*>(p)[k]);   // (all members are doubles)
  if (!finite) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_shape_reward: every weight and parameter must be finite");
  if (!(p->tracking_sigma > 0)) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_shape_reward: tracking_sigma must be > 0");
  if (!(cfg->sim_dt > 0) || !std::isfinite(cfg->sim_dt)) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_shape_reward: sim_dt must be > 0");
  if (cfg->frame_skip < 1) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_shape_reward: frame_skip must be >= 1");
  if (int rc = solo::select_device(device_id)) return rc;
  return ShapeShell::launch("solorl_shape_reward: shape_rows_kernel launch", cfg->robot == SOLORL_ROBOT_SOLO12 ? shape_rows_kernel<1> : shape_rows_kernel<0>, n, stream,
                            reinterpret_cast<const double*>(states), mask, n, actions, done, reinterpret_cast<double*>(mem), reward, terms_out, ep_out, cmd, *p,
                            cfg->sim_dt, cfg->sim_dt * (double)cfg->frame_skip);
}

extern "C" int solorl_shape_reward(const solorl_config* cfg, const solorl_shape_params* p, const solorl_env_state* states, const uint8_t* mask, int n,
                                   const float* actions, const uint8_t* done, solorl_env_shape* mem, float* reward, double* terms_out, double* ep_out,
                                   int device_id, void* stream) {
  return solorl_shape_reward_cmd(cfg, p, states, mask, n, actions, done, mem, reward, terms_out, ep_out, nullptr, device_id, stream);
}
