// solorl_dynamics (include/solorl.h): joint-space mass matrix, bias and gravity forces, foot Jacobians with their Jdot v and foot points
// of a batch of solorl_env_state rows, gfx950.  The arithmetic is csrc/dyn_tensors.hpp (fp64); this file is the memory shape around it
// and the C entry point.  The shape is solorl_kin.hip's.
//
// A row in is 2040 B of which the 37 words pos .. qd are read, a row out is 4800 B: a lane that walked its own rows would touch one
// 8-byte word per 2 KB / 4.8 KB stride with every instruction, and the 324 words of M do not fit a lane's registers.  Instead a
// workgroup of four wavefronts takes DYN_ENVS consecutive rows:
//   1. all lanes copy the rows' heads (37 contiguous words each) into LDS, lane after lane along each row;
//   2. wavefront w runs leg w of the row's arithmetic for every row, lane = row, wavefront 0 the base link after its leg (DynRow
//      parts), reading LDS at immediate offsets and storing every output word there as soon as it exists: M is never held in
//      registers.  The parts are independent up to their shares of the robot's inertia and wrench about pos (16 words each);
//   3. behind a barrier the staged input's place (37 words per row) takes the shares of legs 1 and 2, wavefront 0 adds them to its
//      own (base, leg 0, leg 1, leg 2: the order of env_dynamics), then it takes leg 3's share the same way, and wavefront 0 writes
//      the base's 6 x 6 block, bias[0..5] and gravity[0..5] (dyn_totals);
//   4. all lanes copy the output rows from LDS to memory: with no mask the workgroup's rows are ONE contiguous segment of
//      DYN_ENVS x 4800 B, written 512 B per wave instruction.
// Rows start on 8-byte boundaries only (2040 is an odd multiple of 8), hence 8-byte accesses.
// Residency.  LDS: a row costs (37 + 600) x 8 = 5096 B; DYN_ENVS = 16 rows and their live flags are 81 600 B of static LDS, two
// workgroups 163 200 B of the CU's 163 840.  Registers: the kernel allocates 248 (Solo12) / 224 (Solo8) VGPRs and no AGPRs, so a SIMD
// holds two wavefronts and a CU eight -- two workgroups of four, by both limits: one workgroup's copies beside the other's arithmetic.
// A masked row (mask byte 0) is skipped in all phases: neither read nor written.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dyn_tensors.hpp"

extern "C" int solorl_fail_(int code, const char* msg);

namespace {

constexpr int DYN_ENVS = 16;        // envs per workgroup (solorl_amd/dyn_tensors.py ENVS_PER_WORKGROUP says the same; tests/test_dyn_static.py)
constexpr int DYN_WAVES = 4;        // wavefront w runs leg w of every row of the workgroup; wavefront 0 the base link after it
constexpr int DYN_THREADS = 64 * DYN_WAVES;
constexpr size_t DYN_LDS_BYTES = (size_t)DYN_ENVS * (solo::DYN_IN_WORDS + solo::DYN_OUT_WORDS) * 8 + DYN_ENVS * 4;
static_assert(DYN_ENVS <= 64, "one lane per env in the arithmetic phase");
static_assert(DYN_WAVES + 1 == solo::DYN_PARTS, "four legs and the base");
static_assert(2 * DYN_LDS_BYTES <= 160 * 1024, "two workgroups share the LDS of a CU");
static_assert(2 * solo::DYN_SUM_WORDS <= solo::DYN_IN_WORDS, "two parts' shares at a time take the staged input's place");

template <int ROBOT>
__global__ __launch_bounds__(DYN_THREADS) void dyn_rows_kernel(const double* __restrict__ states, const uint8_t* __restrict__ mask, int n,
                                                                double* __restrict__ out, int urdf, double gravity, double damping) {
  using namespace solo;
  __shared__ double s_in[DYN_ENVS * DYN_IN_WORDS];
  __shared__ double s_out[DYN_ENVS * DYN_OUT_WORDS];
  __shared__ int s_live[DYN_ENVS];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);            // (uniform: the switch below is a scalar branch)
  const int e0 = blockIdx.x * DYN_ENVS;                    // < n (the grid is ceil(n / DYN_ENVS))
  if (t < DYN_ENVS) s_live[t] = (t < n - e0) && (mask == nullptr || mask[e0 + t] != 0);
  __syncthreads();
#pragma unroll 1
  for (int idx = t; idx < DYN_ENVS * DYN_IN_WORDS; idx += DYN_THREADS) {
    const int r = idx / DYN_IN_WORDS, w = idx - r * DYN_IN_WORDS;
    if (s_live[r]) s_in[idx] = states[(size_t)(e0 + r) * KIN_STATE_WORDS + w];
  }
  __syncthreads();
  const bool mine = lane < DYN_ENVS && s_live[lane];       // this lane has a row (the same one in every wavefront)
  const double* in = s_in + lane * DYN_IN_WORDS;
  double* o = s_out + lane * DYN_OUT_WORDS;
  auto ld = [&](int w) { return in[w]; };
  auto st = [&](int w, double v) { o[w] = v; };
  using Row = DynRow<double, ROBOT, decltype(ld), decltype(st)>;
  DynSums<double> S{};                                     // this wavefront's leg; wavefront 0: the base plus its leg
  if (mine) {
    Row row(ld, st, urdf != 0, gravity, damping);
    switch (wave) {
      case 0: row.template part<1>(); break;
      case 1: row.template part<2>(); break;
      case 2: row.template part<3>(); break;
      default: row.template part<4>(); break;
    }
    S = row.S;
    if (wave == 0) {                                       // (after its leg, so that the base's share is not held through it)
      Row base(ld, st, urdf != 0, gravity, damping);
      base.template part<0>();
      dyn_add(base.S, S);
      S = base.S;
    }
  }
  __syncthreads();                                         // every part has read what it needs of s_in: its place is free
  double* slot = s_in + lane * DYN_IN_WORDS;               // this row's two slots of DYN_SUM_WORDS
  auto put = [&](int k, const DynSums<double>& A) {
    double* q = slot + k * DYN_SUM_WORDS;
    q[0] = A.I.m; q[1] = A.I.h.x; q[2] = A.I.h.y; q[3] = A.I.h.z;
    q[4] = A.I.I.xx; q[5] = A.I.I.xy; q[6] = A.I.I.xz; q[7] = A.I.I.yy; q[8] = A.I.I.yz; q[9] = A.I.I.zz;
    q[10] = A.W.a.x; q[11] = A.W.a.y; q[12] = A.W.a.z; q[13] = A.W.l.x; q[14] = A.W.l.y; q[15] = A.W.l.z;
  };
  auto take = [&](int k) {
    const double* q = slot + k * DYN_SUM_WORDS;
    return DynSums<double>{RBI<double>{q[0], mk(q[1], q[2], q[3]), Sym3<double>{q[4], q[5], q[6], q[7], q[8], q[9]}},
                           SV<double>{mk(q[10], q[11], q[12]), mk(q[13], q[14], q[15])}};
  };
  if (mine && (wave == 1 || wave == 2)) put(wave - 1, S);
  __syncthreads();
  if (mine && wave == 0) { dyn_add(S, take(0)); dyn_add(S, take(1)); }
  __syncthreads();
  if (mine && wave == 3) put(0, S);
  __syncthreads();
  if (mine && wave == 0) {
    dyn_add(S, take(0));
    dyn_totals<double>(st, S, gravity);
  }
  __syncthreads();
  double* dst = out + (size_t)e0 * DYN_OUT_WORDS;
#pragma unroll 4
  for (int idx = t; idx < DYN_ENVS * DYN_OUT_WORDS; idx += DYN_THREADS)
    if (s_live[idx / DYN_OUT_WORDS]) dst[idx] = s_out[idx];
}

int select_device(int device_id) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return solorl_fail_(SOLORL_ERR_NODEVICE, "no HIP device available (no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return solorl_fail_(SOLORL_ERR_NODEVICE, "device_id out of range");
  if (hipSetDevice(device_id) != hipSuccess) return solorl_fail_(SOLORL_ERR_HIP, "hipSetDevice");
  return 0;
}

}  // namespace

extern "C" int solorl_dynamics(const solorl_config* cfg, const solorl_env_state* states, const uint8_t* mask, int n, solorl_env_dyn* out,
                               int device_id, void* stream) {
  if (!cfg) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_dynamics: null config");
  if (!states || !out) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_dynamics: null states or out");
  if (n < 1) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_dynamics: n must be >= 1");
  if (cfg->robot != SOLORL_ROBOT_SOLO8 && cfg->robot != SOLORL_ROBOT_SOLO12) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_dynamics: robot must be SOLORL_ROBOT_SOLO8 or SOLORL_ROBOT_SOLO12");
  if (!std::isfinite(cfg->gravity)) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_dynamics: gravity must be finite");
  if (!std::isfinite(cfg->damping) || cfg->damping < 0) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_dynamics: damping must be finite and >= 0");
  if (int rc = select_device(device_id)) return rc;
  const dim3 grid((unsigned)((n - 1) / DYN_ENVS + 1));
  auto kernel = cfg->robot == SOLORL_ROBOT_SOLO12 ? dyn_rows_kernel<1> : dyn_rows_kernel<0>;
  hipLaunchKernelGGL(kernel, grid, dim3(DYN_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const double*>(states), mask, n,
                     reinterpret_cast<double*>(out), cfg->use_urdf_inertia, cfg->gravity, cfg->damping);
  return hipGetLastError() == hipSuccess ? 0 : solorl_fail_(SOLORL_ERR_HIP, "solorl_dynamics: dyn_rows_kernel launch");
}
