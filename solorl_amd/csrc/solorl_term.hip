// solorl_terminate (include/solorl.h, "Early termination"): four early termination rules on a batch of solorl_env_state rows, gfx950.
// The arithmetic is csrc/termination.hpp (fp64 comparisons, host-and-device functions), the memory shape around it csrc/row_batch.hpp
// (why rows are staged through LDS); this file is that shape's numbers for this query, the order of the phases, and the C entry point.
//
// A row in is 2040 B of which 49 words are staged: pos.z and quat (5 contiguous words), q (12), lambda_prev (24) and the row's last 8
// words -- dr, treadmill_y, the word of timestep and the word of contact_mask (treadmill_y is not read: it keeps the tail one segment
// and makes the stride odd).  Nothing goes out as rows: a row's results are single elements of done, reward, fired_out, the info
// arrays and two field-major statistics blocks, each written by the row's own lane -- consecutive lanes, consecutive addresses.
// A workgroup of four wavefronts takes TERM_ENVS = 64 consecutive rows; all 256 lanes stage, then lane t of wavefront 0 is row t.  There
// is no leg to split: a row's arithmetic is a few dozen comparisons and up to 24 divisions, so wavefronts 1..3 are done after staging.
// 49 is odd: the 64 lanes' 8-byte reads at one immediate offset fall on different bank pairs within each half-wavefront.
// Residency: 64 x (49 x 8 + 4) = 25 344 B of static LDS, six workgroups per CU by LDS; the register count ("Early
// termination") allows eight wavefronts per SIMD, so LDS decides.  The launch is latency-sized: at 65 536 rows it moves 26 MB.
#include <cmath>

#include "row_batch.hpp"
#include "termination.hpp"

namespace {

constexpr int TERM_ENVS = 64;       // rows per workgroup: every lane of wavefront 0 has a row
using TermShell = solo::RowBatch<TERM_ENVS, solo::TERM_IN_WORDS, 0, 256, 4>;
static_assert(solo::TERM_IN_WORDS == 49 && solo::TERM_IN_WORDS % 2 == 1, "an odd row stride: lane = row reads at one offset are conflict-free");
static_assert(TermShell::LDS_BYTES == (size_t)TERM_ENVS * (solo::TERM_IN_WORDS * 8 + 4) && 6 * TermShell::LDS_BYTES <= 160 * 1024, "static LDS of the kernel");

template <int ROBOT>
__global__ __launch_bounds__(256) void term_rows_kernel(const double* __restrict__ states, const uint8_t* __restrict__ mask, int n, solorl_termination P,
                                                        double sim_dt, uint8_t* __restrict__ done, float* __restrict__ reward,
                                                        uint8_t* __restrict__ fired_out, solorl_info_soa info, float* __restrict__ term_stats) {
  using namespace solo;
  __shared__ double s_in[TERM_ENVS * TERM_IN_WORDS];
  __shared__ int s_live[TERM_ENVS];
  const RowLane me = TermShell::rows_lane();
  TermShell::rows_live(s_live, mask, n);
  TermShell::rows_stage_in(s_in, s_live, states, [](int w) { return term_in_word(w); });
  if (me.wave != 0 || !TermShell::rows_mine(s_live, me.lane)) return;
  const double* row = s_in + me.lane * TERM_IN_WORDS;
  const size_t i = (size_t)TermShell::first_row() + me.lane;          // < n: the row is live
  terminate_row<ROBOT>([&](int w) { return row[term_staged_word(w)]; }, P, sim_dt, (size_t)n, i, done + i, reward + i, fired_out + i, &info, term_stats);
}

}  // namespace

extern "C" int solorl_terminate(const solorl_config* cfg, const solorl_termination* p, const solorl_env_state* states, const uint8_t* mask, int n,
                                uint8_t* done, float* reward, uint8_t* fired_out, const solorl_info_soa* info, float* term_stats, int device_id,
                                void* stream) {
  const char* fn = "solorl_terminate";
  if (int rc = solo::rows_check_args(fn, cfg, states, fired_out, n)) return rc;
  if (!p || !done || !reward) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_terminate: null params, done or reward");
  if (const char* what = solo::term_refusal(*p, cfg->robot, cfg->sim_dt)) {
    char msg[128];
    std::snprintf(msg, sizeof(msg), "%s: %s", fn, what);
    return solorl_fail_(SOLORL_ERR_INVALID, msg);
  }
  if (int rc = solo::select_device(device_id)) return rc;
  const solorl_info_soa none{};
  return TermShell::launch("solorl_terminate: term_rows_kernel launch", cfg->robot == SOLORL_ROBOT_SOLO12 ? term_rows_kernel<1> : term_rows_kernel<0>, n, stream,
                           reinterpret_cast<const double*>(states), mask, n, *p, cfg->sim_dt, done, reward, fired_out, info ? *info : none, term_stats);
}
