// row_batch.hpp -- the shell of a row query: a kernel that derives one output row from every solorl_env_state row of a batch
// (solorl_kin.hip, solorl_dyn.hip), and what the C entry points around such kernels share.  The arithmetic is the caller's.
//
// Why rows are staged: a state row is 2040 B of which the head is read, an output row several KB; a lane that walked its own rows would
// touch one 8-byte word per stride with every instruction.  So a workgroup takes ENVS consecutive rows, all lanes copy the words that
// are read into LDS, lane after lane along each row (rows_stage_in), the arithmetic reads and writes LDS at immediate offsets, and all
// lanes copy the output rows out (rows_stage_out): with no mask they are ONE contiguous segment, written 512 B per wave instruction.
// Why 8-byte accesses: rows start on 8-byte boundaries only (2040 is an odd multiple of 8).
// Why a wavefront per leg: a row's arithmetic is a serial fp64 chain of thousands of instructions and the LDS bounds the rows in flight,
// not the lanes; split by leg (lane = row, wavefront = leg, rows_lane) the chain is a quarter as long.  The base link's part goes to
// wavefront 0, before or after its leg, and the parts' shares of the robot's sums are exchanged through the staged input's place:
// both are the caller's choreography.  A masked row (mask byte 0) is skipped in all phases: neither read nor written.
// A third query: its arithmetic as a struct with part<0..4>() beside KinRow / DynRow, a .hip file with its ENVS chosen so that two
// workgroups fit a CU by LDS and by registers, a kernel made of these pieces, and an entry point made of rows_check_args and launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/solorl.h"

extern "C" int solorl_fail_(int code, const char* msg);

namespace solo {

struct RowLane { int lane, wave; };                  // lane = row of the workgroup, wavefront = leg

// UNROLL_IN: the stage-in loop's unroll factor, chosen per kernel with its register count in view
template <int ENVS, int IN_WORDS, int OUT_WORDS, int THREADS, int UNROLL_IN> struct RowBatch {
  static constexpr size_t LDS_BYTES = (size_t)ENVS * (IN_WORDS + OUT_WORDS) * 8 + ENVS * 4;
  static_assert(ENVS <= 64 && THREADS == 4 * 64, "one lane per env and one wavefront per leg in the arithmetic phase");
  static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups share the LDS of a CU");

  static __device__ __forceinline__ int first_row() { return blockIdx.x * ENVS; }     // < n (the grid is ceil(n / ENVS))
  static __device__ __forceinline__ void rows_live(int* s_live, const uint8_t* mask, int n) {
    const int t = threadIdx.x, e0 = first_row();
    if (t < ENVS) s_live[t] = (t < n - e0) && (mask == nullptr || mask[e0 + t] != 0);
    __syncthreads();
  }
  // word(w): the state row's word that staged word w holds
  template <typename MAP> static __device__ __forceinline__ void rows_stage_in(double* s_in, const int* s_live, const double* states, MAP word) {
#pragma unroll UNROLL_IN
    for (int idx = threadIdx.x; idx < ENVS * IN_WORDS; idx += THREADS) {
      const int r = idx / IN_WORDS, w = idx - r * IN_WORDS;
      if (s_live[r]) s_in[idx] = states[(size_t)(first_row() + r) * (sizeof(solorl_env_state) / 8) + word(w)];
    }
    __syncthreads();
  }
  static __device__ __forceinline__ RowLane rows_lane() {
    const int t = threadIdx.x;
    return {t & 63, __builtin_amdgcn_readfirstlane(t >> 6)};     // (wave is uniform: run_leg_part is a scalar branch)
  }
  // whether this lane has a live row (the same one in every wavefront); after rows_live
  static __device__ __forceinline__ bool rows_mine(const int* s_live, int lane) { return lane < ENVS && s_live[lane]; }
  static __device__ __forceinline__ void rows_stage_out(double* out, const double* s_out, const int* s_live) {
    double* dst = out + (size_t)first_row() * OUT_WORDS;
#pragma unroll 4
    for (int idx = threadIdx.x; idx < ENVS * OUT_WORDS; idx += THREADS)
      if (s_live[idx / OUT_WORDS]) dst[idx] = s_out[idx];
  }
  // the grid, the launch and its error; what: "<function>: <kernel> launch"
  template <typename K, typename... A> static int launch(const char* what, K kernel, int n, void* stream, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n - 1) / ENVS + 1)), dim3(THREADS), 0, (hipStream_t)stream, args...);
    return hipGetLastError() == hipSuccess ? 0 : solorl_fail_(SOLORL_ERR_HIP, what);
  }
};

// leg `wave` of a row: part 1 + wave of a KinRow / DynRow
template <typename ROW> __device__ __forceinline__ void run_leg_part(int wave, ROW& row) {
  switch (wave) {
    case 0: row.template part<1>(); break;
    case 1: row.template part<2>(); break;
    case 2: row.template part<3>(); break;
    default: row.template part<4>(); break;
  }
}

inline int select_device(int device_id) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return solorl_fail_(SOLORL_ERR_NODEVICE, "no HIP device available (no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return solorl_fail_(SOLORL_ERR_NODEVICE, "device_id out of range");
  if (hipSetDevice(device_id) != hipSuccess) return solorl_fail_(SOLORL_ERR_HIP, "hipSetDevice");
  return 0;
}

// the arguments every row query shares; fn: the entry point's name, for the message
inline int rows_check_args(const char* fn, const solorl_config* cfg, const void* states, const void* out, int n) {
  const char* what = !cfg ? "null config" : !states || !out ? "null states or out" : n < 1 ? "n must be >= 1"
                     : cfg->robot != SOLORL_ROBOT_SOLO8 && cfg->robot != SOLORL_ROBOT_SOLO12 ? "robot must be SOLORL_ROBOT_SOLO8 or SOLORL_ROBOT_SOLO12" : nullptr;
  if (!what) return 0;
  char msg[128];
  std::snprintf(msg, sizeof(msg), "%s: %s", fn, what);
  return solorl_fail_(SOLORL_ERR_INVALID, msg);
}

}  // namespace solo
