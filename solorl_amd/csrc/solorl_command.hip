// solorl_commands (include/solorl.h, "Velocity commands"): per-env velocity commands drawn from ranges and resampled on a per-env
// countdown, and the observation rows widened by the three command words the policy is to see -- gfx950.  The arithmetic is
// csrc/command.hpp, host-and-device functions; this file is the kernel's thread mapping and the C entry point.  The kernel does not know
// the engine: it works on the caller's [n][D] and [n][D + 3] float arrays and on caller-owned per-env memory.
//
// Small and memory-bound: a row is read once and written once, two Philox blocks per DRAW (not per call) are all the arithmetic.  A
// workgroup of four wavefronts takes CMD_ROWS = 64 consecutive envs.  Lane t of wavefront 0 is env t: it reads the env's 32-byte memory
// row, decides, draws, and writes the memory row, cmd_out and the row's three command words.  All 256 threads then move the
// workgroup's 64 x D observation words, which are ONE contiguous piece of obs_in, consecutive threads on consecutive words; the two
// parts touch different words, so no barrier stands between them.  No LDS, no scratch, no atomics.
//
// Widths.  The read side: a workgroup's piece of obs_in starts 64 D floats = 256 D bytes behind the one before it, so it is 16-byte
// aligned for every D whenever obs_in is, and holds 16 D whole 16-byte words: it is read as 16-byte words (WIDE), which do not care
// where a row ends.  The write side: row r of obs_out starts 4 r (D + 3) bytes in -- whatever the base, the starts of consecutive rows
// run through several residues mod 16 (all four when D is even, two when D % 4 == 3; with D % 4 == 1 they share one, but then a row of
// the INPUT starts at every residue), so a 16-byte word of the input never maps onto an aligned 16-byte word of the output for every
// row: every output word goes out as a 4-byte store at its own address (four stores per 16-byte load, neighbouring lanes 16 bytes apart:
// the four instructions fill the same lines between them).  An obs_in that is not 16-byte aligned is read word by word, lane = word,
// and written likewise, consecutive lanes on consecutive addresses but for the 12-byte gap at a row end; the values are the same.
// Measured ("Velocity commands"): at 65 536 envs the two read paths cannot be told apart; the call is launch-latency sized.
#include <cmath>
#include <cstddef>

#include "command.hpp"
#include "row_batch.hpp"

namespace {

constexpr int CMD_ROWS = 64, CMD_THREADS = 256;

struct Walk {                     // (row, column) of a word of the workgroup's piece, advanced by a fixed number of words
  int r, c;
  __device__ __forceinline__ void step(int dr, int dc, int D) {
    r += dr;
    c += dc;
    if (c >= D) { c -= D; r++; }
  }
};

// The workgroup's piece: `rows` (<= CMD_ROWS) rows of `in` (D floats each, dense) to rows of D + 3 floats at `out`; mask: the piece's
// bytes or nullptr.  WIDE: 16-byte loads (in is 16-byte aligned); a 16-byte word that holds a word of a masked row or of a row past the
// end is read word by word, its live words only.  (dr, dc) = (W / D, W % D) for the W = 1024 (WIDE) or 256 words between a thread's
// consecutive accesses: one division per thread, none in the loop.
template <bool WIDE, bool MASKED>
__device__ __forceinline__ void rows_widen(const uint8_t* __restrict__ mask, int rows, int D, int dr, int dc, const float* __restrict__ in,
                                           float* __restrict__ out) {
  const int t = threadIdx.x, O = D + 3;
  auto live = [&](int r) { return r < rows && (!MASKED || mask[r] != 0); };
  if (WIDE) {
    Walk at{4 * t / D, 0};
    at.c = 4 * t - at.r * D;
#pragma unroll 2
    for (int q = t; q < CMD_ROWS / 4 * D && at.r < rows; q += CMD_THREADS) {
      Walk w[4];
      w[0] = at;
#pragma unroll
      for (int j = 1; j < 4; j++) { w[j] = w[j - 1]; w[j].step(0, 1, D); }
      const bool all = live(w[0].r) && live(w[1].r) && live(w[2].r) && live(w[3].r);
      if (all) {
        const float4 x = *reinterpret_cast<const float4*>(in + 4 * q);
        out[(size_t)w[0].r * O + w[0].c] = x.x;
        out[(size_t)w[1].r * O + w[1].c] = x.y;
        out[(size_t)w[2].r * O + w[2].c] = x.z;
        out[(size_t)w[3].r * O + w[3].c] = x.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (live(w[j].r)) out[(size_t)w[j].r * O + w[j].c] = in[4 * q + j];
      }
      at.step(dr, dc, D);
    }
  } else {
    Walk at{t / D, 0};
    at.c = t - at.r * D;
#pragma unroll 4
    for (int k = t; k < CMD_ROWS * D && at.r < rows; k += CMD_THREADS) {
      if (live(at.r)) out[(size_t)at.r * O + at.c] = in[k];
      at.step(dr, dc, D);
    }
  }
}

template <bool WIDE>
__global__ __launch_bounds__(CMD_THREADS) void command_kernel(solo::CommandParams P, const uint8_t* __restrict__ mask, const uint8_t* __restrict__ restart,
                                                              int n, int D, int dr, int dc, solo::CommandRow* __restrict__ mem,
                                                              const float* __restrict__ obs_in, float* __restrict__ obs_out, double* __restrict__ cmd_out) {
  using namespace solo;
  const long long first = (long long)blockIdx.x * CMD_ROWS;
  const int rows = n - first < CMD_ROWS ? (int)(n - first) : CMD_ROWS;
  if ((int)threadIdx.x < rows) {                                // wavefront 0, lane = env
    const long long i = first + threadIdx.x;
    if (mask == nullptr || mask[i] != 0)
      command_env(P, P.key.id0 + i, restart != nullptr && restart[i] != 0, mem + i, obs_out ? obs_out + (size_t)i * (D + 3) + D : nullptr,
                  cmd_out ? cmd_out + (size_t)i * 3 : nullptr);
  }
  if (obs_out == nullptr) return;
  const float* in = obs_in + (size_t)first * D;
  float* out = obs_out + (size_t)first * (D + 3);
  if (mask) rows_widen<WIDE, true>(mask + first, rows, D, dr, dc, in, out);
  else rows_widen<WIDE, false>(nullptr, rows, D, dr, dc, in, out);
}

}  // namespace

extern "C" int solorl_commands(const solorl_command_params* p, const uint8_t* mask, const uint8_t* restart, int n, solorl_env_command* mem,
                               const float* obs_in, float* obs_out, double* cmd_out, int device_id, void* stream) {
  static_assert(sizeof(solorl_env_command) == sizeof(solo::CommandRow) && sizeof(solorl_env_command) == 32 &&
                offsetof(solorl_env_command, countdown) == offsetof(solo::CommandRow, countdown) &&
                offsetof(solorl_env_command, draws) == offsetof(solo::CommandRow, draws) && offsetof(solorl_env_command, draws) == 28,
                "command.hpp's CommandRow is solorl_env_command");
  static_assert((CMD_ROWS * sizeof(float)) % 16 == 0 && CMD_ROWS % 4 == 0 && CMD_ROWS <= 64, "a workgroup's piece of obs_in: whole 16-byte words; its envs: one wavefront");
  if (!p || !mem) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_commands: null params or mem");
  if ((obs_in == nullptr) != (obs_out == nullptr)) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_commands: obs_in and obs_out must both be given or both be NULL");
  if (n < 1) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_commands: n must be >= 1");
  if (p->obs_dim < 1 || p->obs_dim > solo::CHANNEL_MAX_OBS) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_commands: obs_dim must be 1..210");
  for (int k = 0; k < 3; k++) {
    if (!std::isfinite(p->lo[k]) || !std::isfinite(p->hi[k]) || !(p->lo[k] <= p->hi[k]))
      return solorl_fail_(SOLORL_ERR_INVALID, "solorl_commands: every range must be finite with lo <= hi");
    if (!std::isfinite(p->obs_scale[k])) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_commands: every obs_scale must be finite");
  }
  if (!(p->zero_prob >= 0.0 && p->zero_prob <= 1.0)) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_commands: zero_prob must lie in [0, 1]");
  if (!std::isfinite(p->min_lin_norm) || p->min_lin_norm < 0.0) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_commands: min_lin_norm must be finite and >= 0");
  if (p->interval_min < 1 || p->interval_min > p->interval_max || p->interval_max > solo::COMMAND_INTERVAL_MAX)
    return solorl_fail_(SOLORL_ERR_INVALID, "solorl_commands: the interval range must satisfy 1 <= interval_min <= interval_max <= 1 << 20");
  if (int rc = solo::select_device(device_id)) return rc;
  solo::CommandParams P;
  P.key = {(unsigned)p->seed, (unsigned)(p->seed >> 32), (long long)p->env_id_offset};
  for (int k = 0; k < 3; k++) { P.lo[k] = p->lo[k]; P.hi[k] = p->hi[k]; P.obs_scale[k] = p->obs_scale[k]; }
  P.zero_prob = p->zero_prob;
  P.min_lin_norm = p->min_lin_norm;
  P.interval_min = p->interval_min;
  P.span = (unsigned)(p->interval_max - p->interval_min + 1);
  const int D = p->obs_dim;
  const bool wide = reinterpret_cast<uintptr_t>(obs_in) % 16 == 0;
  const int W = wide ? 4 * CMD_THREADS : CMD_THREADS;       // words between a thread's consecutive accesses
  hipLaunchKernelGGL(wide ? command_kernel<true> : command_kernel<false>, dim3((unsigned)((n - 1) / CMD_ROWS + 1)), dim3(CMD_THREADS), 0, (hipStream_t)stream, P,
                     mask, restart, n, D, W / D, W % D, reinterpret_cast<solo::CommandRow*>(mem), obs_in, obs_out, cmd_out);
  return hipGetLastError() == hipSuccess ? 0 : solorl_fail_(SOLORL_ERR_HIP, "solorl_commands: command_kernel launch");
}
