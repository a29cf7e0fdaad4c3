// solorl_randomize_reset (include/solorl.h, "Randomised initial states"): joint angles and velocities, base velocity, heading, roll and
// pitch of a batch of solorl_env_state rows drawn from a Philox stream per env, and the robot placed on the ground, in place, gfx950.
// The arithmetic is csrc/reset_random.hpp (fp64), the memory shape around it csrc/row_batch.hpp (why rows are staged through LDS, a
// wavefront per leg); this file is that shape's numbers for this query, the order of the phases, and the C entry point.
//
// A row is 2040 B of which the head is staged in: pos .. qd, 37 contiguous words.  A workgroup of four wavefronts takes RESET_ENVS
// consecutive rows, lane = row in every wavefront.  Phase 1, the draws: the nine Philox blocks of a row are independent, so wavefront 0
// takes blocks 6, 7, 8 (base velocities and the three angles) and turns the quaternion, wavefronts 1, 2, 3 take the joint blocks
// (0, 3), (1, 4), (2, 5): no two wavefronts write the same word.  Behind a barrier, phase 2 (only with place_on_ground): wavefront w
// runs leg w of the NEW pose (a KinRow whose store keeps the minimum of the support points' z and nothing else), wavefront 0 the base's
// twelve points before its leg; the four minima go through LDS ([part][row]: consecutive lanes, consecutive words), wavefront 0 lifts
// pos.z.  Then all lanes copy out the words that may have changed: the 37 head words, and when the pose can change the 24 lambda_prev
// words (zeros) and the contact_mask word (bits 0..23 cleared).  Nothing else of a row is written; count[i] is read by every
// wavefront in phase 1 and written by wavefront 0 behind the barrier.
// 37 is odd: the 64 lanes' 8-byte accesses at one immediate offset fall on different bank pairs within each half-wavefront.
// Residency, by both limits (read from the code object, DESIGN.md section 4 "Randomised initial states").  LDS: 64 x (37 + 4) x 8 B +
// the live flags = 21 248 B of static LDS, seven workgroups per CU (148 736 of 160 KB).  Registers: a leg is KinRow's chain without its
// stores, velocities and sums, 52 VGPRs (Solo12) / 53 (Solo8), no AGPRs, no scratch: eight wavefronts per SIMD would fit, so LDS
// decides -- seven workgroups, far more than the two the shell asks for.  RESET_ENVS = 64: every lane of a wavefront has a row; more
// rows per workgroup would need a second row per lane.  The launch is latency-sized: at 65 536 rows it moves about 50 MB.
#include <cmath>

#include "reset_random.hpp"
#include "row_batch.hpp"

namespace {

constexpr int RESET_ENVS = 64;      // rows per workgroup (solorl_amd/reset_random.py ENVS_PER_WORKGROUP says the same)
constexpr int RESET_WAVES = 4;      // phase 1: a share of the blocks each; phase 2: wavefront w runs leg w, wavefront 0 the base before it
using ResetShell = solo::RowBatch<RESET_ENVS, solo::RESET_HEAD_WORDS, RESET_WAVES, 64 * RESET_WAVES, 2>;
static_assert(solo::RESET_HEAD_WORDS % 2 == 1, "an odd row stride: lane = row accesses at one offset are conflict-free");
static_assert(ResetShell::LDS_BYTES == (size_t)RESET_ENVS * ((solo::RESET_HEAD_WORDS + RESET_WAVES) * 8 + 4) && ResetShell::LDS_BYTES == 21248, "static LDS of the kernel");

// WORDS words from word `first` on of every live row: value(r, w) -> the row in global memory, lane after lane along each row
template <int WORDS, typename VAL> __device__ __forceinline__ void rows_copy_back(double* rows, int first, const int* s_live, VAL value) {
#pragma unroll 2
  for (int idx = threadIdx.x; idx < RESET_ENVS * WORDS; idx += 64 * RESET_WAVES) {
    const int r = idx / WORDS, w = idx - r * WORDS;
    if (s_live[r]) rows[(size_t)(ResetShell::first_row() + r) * solo::STATE_WORDS + first + w] = value(r, w);
  }
}

template <int ROBOT>
__global__ __launch_bounds__(64 * RESET_WAVES) void reset_rows_kernel(double* rows, const uint8_t* __restrict__ mask, int n, uint32_t* count,
                                                                       solorl_reset_randomization P, double joint_limit) {
  using namespace solo;
  __shared__ double s_in[RESET_ENVS * RESET_HEAD_WORDS];
  __shared__ double s_min[RESET_WAVES * RESET_ENVS];
  __shared__ int s_live[RESET_ENVS];
  const RowLane me = ResetShell::rows_lane();
  ResetShell::rows_live(s_live, mask, n);
  ResetShell::rows_stage_in(s_in, s_live, rows, [](int w) { return w; });
  const bool mine = ResetShell::rows_mine(s_live, me.lane);
  double* row = s_in + me.lane * RESET_HEAD_WORDS;
  auto ld = [&](int w) { return row[w]; };
  auto st = [&](int w, double v) { row[w] = v; };
  const size_t i = (size_t)ResetShell::first_row() + me.lane;          // < n where the row is live
  unsigned k = 0u;
  if (mine) {
    k = count[i];
    const long long gid = (long long)P.env_id_offset + (long long)i;
    ResetAngles A{0.0, 0.0, 0.0};
    switch (me.wave) {
      case 0:
        reset_draw_block<ROBOT, 6>(ld, st, P, joint_limit, gid, k, A);
        reset_draw_block<ROBOT, 7>(ld, st, P, joint_limit, gid, k, A);
        reset_draw_block<ROBOT, 8>(ld, st, P, joint_limit, gid, k, A);
        if (reset_turns(P)) reset_orient(ld, st, A);
        break;
      case 1: reset_draw_block<ROBOT, 0>(ld, st, P, joint_limit, gid, k, A); reset_draw_block<ROBOT, 3>(ld, st, P, joint_limit, gid, k, A); break;
      case 2: reset_draw_block<ROBOT, 1>(ld, st, P, joint_limit, gid, k, A); reset_draw_block<ROBOT, 4>(ld, st, P, joint_limit, gid, k, A); break;
      default: reset_draw_block<ROBOT, 2>(ld, st, P, joint_limit, gid, k, A); reset_draw_block<ROBOT, 5>(ld, st, P, joint_limit, gid, k, A); break;
    }
  }
  __syncthreads();                                         // the new pose of every row is in LDS; every wavefront has read count
  if (mine && me.wave == 0) count[i] = k + 1u;
  if (P.place_on_ground != 0) {                            // (uniform: a launch argument)
    if (mine) {
      double zmin = __builtin_inf();
      auto keep = reset_zmin_store<ROBOT>(zmin);
      auto rd = reset_head_reader(ld);
      using Row = KinRow<double, ROBOT, decltype(rd), decltype(keep)>;
      if (me.wave == 0) {
        Row base(rd, keep, 0, false, 1.0, 0.0);
        base.template part<0>();
      }
      Row leg(rd, keep, 0, false, 1.0, 0.0);
      run_leg_part(me.wave, leg);
      s_min[me.wave * RESET_ENVS + me.lane] = zmin;
    }
    __syncthreads();
    if (mine && me.wave == 0) {
      const double zmin = fmin(fmin(s_min[me.lane], s_min[RESET_ENVS + me.lane]), fmin(s_min[2 * RESET_ENVS + me.lane], s_min[3 * RESET_ENVS + me.lane]));
      row[STATE_SW(pos) + 2] = reset_lift(row[STATE_SW(pos) + 2], P.clearance, zmin);
    }
    __syncthreads();
  }
  rows_copy_back<RESET_HEAD_WORDS>(rows, 0, s_live, [&](int r, int w) { return s_in[r * RESET_HEAD_WORDS + w]; });
  if (reset_pose_changes<ROBOT>(P)) {
    rows_copy_back<RESET_LAMBDA_WORDS>(rows, STATE_SW(lambda_prev), s_live, [](int, int) { return 0.0; });
    if (threadIdx.x < RESET_ENVS && s_live[threadIdx.x]) {  // the contact_mask word: the row's own lane, its other bits kept
      double* word = rows + (size_t)(ResetShell::first_row() + threadIdx.x) * STATE_WORDS + RESET_MASK_WORD;
      uint32_t m[2];
      __builtin_memcpy(m, word, sizeof(m));
      m[0] &= RESET_MASK_KEEP;
      __builtin_memcpy(word, m, sizeof(m));
    }
  }
}

}  // namespace

extern "C" int solorl_randomize_reset(const solorl_config* cfg, const solorl_reset_randomization* p, solorl_env_state* rows, const uint8_t* mask,
                                      uint32_t* count, int n, int device_id, void* stream) {
  const char* fn = "solorl_randomize_reset";
  if (int rc = solo::rows_check_args(fn, cfg, rows, count, n)) return rc;
  if (!p) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_randomize_reset: null params");
  if (const char* what = solo::reset_refusal(*p, cfg->joint_limit)) {
    char msg[128];
    std::snprintf(msg, sizeof(msg), "%s: %s", fn, what);
    return solorl_fail_(SOLORL_ERR_INVALID, msg);
  }
  if (int rc = solo::select_device(device_id)) return rc;
  return ResetShell::launch("solorl_randomize_reset: reset_rows_kernel launch", cfg->robot == SOLORL_ROBOT_SOLO12 ? reset_rows_kernel<1> : reset_rows_kernel<0>, n,
                            stream, reinterpret_cast<double*>(rows), mask, n, count, *p, cfg->joint_limit);
}
