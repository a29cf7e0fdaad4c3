// solorl_kinematics (include/solorl.h): link poses, support points of the collision primitives with their velocities and normal
// forces, centre of mass, energy and momentum of a batch of solorl_env_state rows, gfx950.  The arithmetic is csrc/kinematics.hpp
// (fp64); this file is the memory shape around it and the C entry point.
//
// A row in is 2040 B of which 74 words are read, a row out is 3640 B: a lane that walked its own rows would touch one 8-byte word
// per 2 KB / 3.6 KB stride with every instruction.  Instead a workgroup of four wavefronts takes KIN_ENVS consecutive rows:
//   1. all lanes copy the rows' head (pos .. lambda_prev, 73 contiguous words) and their contact_mask word into LDS, lane after lane
//      along each row: every wave instruction reads whole contiguous segments;
//   2. wavefront w runs leg w of the row's arithmetic for every row, lane = row, wavefront 0 the base with its twelve points before
//      its leg (KinRow parts; the base is about a ninth of a leg's work), reading and writing LDS at immediate offsets (row strides
//      of 148 and 910 dwords: of the eighteen lanes, rows 16 and 17 share banks with rows 0 and 1, the others fall on banks of their
//      own).  The parts are independent up to their shares of the link sums, which the wavefronts leave where the staged input was
//      (after a barrier); wavefront 0 adds them in a fixed order and writes the totals (kin_totals);
//   3. all lanes copy the output rows from LDS to memory: with no mask the workgroup's rows are ONE contiguous segment of
//      KIN_ENVS x 3640 B, written 512 B per wave instruction.
// Rows start on 8-byte boundaries only (2040 and 3640 are odd multiples of 8), hence 8-byte accesses.
// Residency, by both limits.  Registers: the kernel allocates 216 (Solo12) / 184 (Solo8) VGPRs, so a SIMD holds two wavefronts and a
// CU eight -- two workgroups of four.  LDS: a row costs (74 + 455) x 8 = 4232 B; KIN_ENVS = 18 rows are 76.2 KB of static LDS, two
// workgroups 152 KB of the CU's 160.  The two limits meet at two workgroups of 18 rows: 36 rows in flight per CU, one workgroup's
// copies beside the other's arithmetic.  (A fifth wavefront for the base, or more registers, would leave room for one workgroup only.)
// Why a wavefront per leg: a row's arithmetic is a serial fp64 chain of ~9000 instructions, 24 calls of sincos_call among them, and
// the LDS bounds the rows in flight, not the lanes; split by leg the chain is a quarter as long.
// A masked row (mask byte 0) is skipped in all phases: neither read nor written.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "kinematics.hpp"

extern "C" int solorl_fail_(int code, const char* msg);

namespace {

constexpr int KIN_ENVS = 18;        // envs per workgroup (solorl_amd/kinematics.py ENVS_PER_WORKGROUP says the same; tests/test_kin_static.py)
constexpr int KIN_WAVES = 4;        // wavefront w runs leg w of every row of the workgroup; wavefront 0 the base (a ninth of a leg's work) before it
constexpr int KIN_THREADS = 64 * KIN_WAVES;
constexpr size_t KIN_LDS_BYTES = (size_t)KIN_ENVS * (solo::KIN_IN_WORDS + solo::KIN_OUT_WORDS) * 8 + KIN_ENVS * 4;
static_assert(KIN_ENVS <= 64, "one lane per env in the arithmetic phase");
static_assert(KIN_WAVES + 1 == solo::KIN_PARTS, "four legs and the base");
static_assert(2 * KIN_LDS_BYTES <= 160 * 1024, "two workgroups share the LDS of a CU");
static_assert(solo::KIN_PARTS * KIN_ENVS * solo::KIN_SUM_WORDS <= KIN_ENVS * solo::KIN_IN_WORDS, "the parts' sums take the staged input's place");

template <int ROBOT>
__global__ __launch_bounds__(KIN_THREADS) void kin_rows_kernel(const double* __restrict__ states, const uint8_t* __restrict__ mask, int n,
                                                                double* __restrict__ out, int urdf, double sim_dt, double gravity) {
  using namespace solo;
  __shared__ double s_in[KIN_ENVS * KIN_IN_WORDS];
  __shared__ double s_out[KIN_ENVS * KIN_OUT_WORDS];
  __shared__ int s_live[KIN_ENVS];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);            // (uniform: the switch below is a scalar branch)
  const int e0 = blockIdx.x * KIN_ENVS;                    // < n (the grid is ceil(n / KIN_ENVS))
  if (t < KIN_ENVS) s_live[t] = (t < n - e0) && (mask == nullptr || mask[e0 + t] != 0);
  __syncthreads();
#pragma unroll 2
  for (int idx = t; idx < KIN_ENVS * KIN_IN_WORDS; idx += KIN_THREADS) {
    const int r = idx / KIN_IN_WORDS, w = idx - r * KIN_IN_WORDS;
    if (s_live[r]) s_in[idx] = states[(size_t)(e0 + r) * KIN_STATE_WORDS + (w < KIN_IN_HEAD_WORDS ? w : KIN_IN_MASK_WORD)];
  }
  __syncthreads();
  const bool mine = lane < KIN_ENVS && s_live[lane];       // this lane has a row (the same one in every wavefront)
  const double* in = s_in + lane * KIN_IN_WORDS;
  double* o = s_out + lane * KIN_OUT_WORDS;
  auto ld = [&](int w) { return in[w]; };
  auto st = [&](int w, double v) { o[w] = v; };
  using Row = KinRow<double, ROBOT, decltype(ld), decltype(st)>;
  KinSums<double> S{}, S0{};                               // this wavefront's leg; wavefront 0: the base as well
  if (mine) {
    // (the staged row keeps the head's word offsets; the contact_mask word sits behind it: bits are copied, never converted)
    int cmask;
    __builtin_memcpy(&cmask, in + KIN_IN_HEAD_WORDS, sizeof(cmask));
    if (wave == 0) {
      Row base(ld, st, cmask, urdf != 0, sim_dt, gravity);
      base.template part<0>();
      S0 = base.S;
    }
    Row row(ld, st, cmask, urdf != 0, sim_dt, gravity);
    switch (wave) {
      case 0: row.template part<1>(); break;
      case 1: row.template part<2>(); break;
      case 2: row.template part<3>(); break;
      default: row.template part<4>(); break;
    }
    S = row.S;
  }
  __syncthreads();                                         // every part has read what it needs of s_in: its place is free
  auto put = [&](int part, const KinSums<double>& A) {
    double* sums = s_in + (part * KIN_ENVS + lane) * KIN_SUM_WORDS;
    sums[0] = A.KE; sums[1] = A.PE; sums[2] = A.M; sums[3] = A.P.x; sums[4] = A.P.y; sums[5] = A.P.z;
    sums[6] = A.Lm.x; sums[7] = A.Lm.y; sums[8] = A.Lm.z; sums[9] = A.MC.x; sums[10] = A.MC.y; sums[11] = A.MC.z;
  };
  if (mine) {
    put(1 + wave, S);
    if (wave == 0) put(0, S0);
  }
  __syncthreads();
  if (wave == 0 && mine) {
    KinSums<double> P[KIN_PARTS];
#pragma unroll
    for (int k = 0; k < KIN_PARTS; k++) {
      const double* q = s_in + (k * KIN_ENVS + lane) * KIN_SUM_WORDS;
      P[k] = KinSums<double>{q[0], q[1], q[2], mk(q[3], q[4], q[5]), mk(q[6], q[7], q[8]), mk(q[9], q[10], q[11])};
    }
    kin_totals<double>(st, P);
  }
  __syncthreads();
  double* dst = out + (size_t)e0 * KIN_OUT_WORDS;
#pragma unroll 4
  for (int idx = t; idx < KIN_ENVS * KIN_OUT_WORDS; idx += KIN_THREADS)
    if (s_live[idx / KIN_OUT_WORDS]) dst[idx] = s_out[idx];
}

int select_device(int device_id) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return solorl_fail_(SOLORL_ERR_NODEVICE, "no HIP device available (no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return solorl_fail_(SOLORL_ERR_NODEVICE, "device_id out of range");
  if (hipSetDevice(device_id) != hipSuccess) return solorl_fail_(SOLORL_ERR_HIP, "hipSetDevice");
  return 0;
}

}  // namespace

extern "C" int solorl_kinematics(const solorl_config* cfg, const solorl_env_state* states, const uint8_t* mask, int n, solorl_env_kin* out,
                                 int device_id, void* stream) {
  if (!cfg) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_kinematics: null config");
  if (!states || !out) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_kinematics: null states or out");
  if (n < 1) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_kinematics: n must be >= 1");
  if (cfg->robot != SOLORL_ROBOT_SOLO8 && cfg->robot != SOLORL_ROBOT_SOLO12) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_kinematics: robot must be SOLORL_ROBOT_SOLO8 or SOLORL_ROBOT_SOLO12");
  if (!(cfg->sim_dt > 0) || !std::isfinite(cfg->sim_dt)) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_kinematics: sim_dt must be > 0");
  if (!std::isfinite(cfg->gravity)) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_kinematics: gravity must be finite");
  if (int rc = select_device(device_id)) return rc;
  const dim3 grid((unsigned)((n - 1) / KIN_ENVS + 1));
  auto kernel = cfg->robot == SOLORL_ROBOT_SOLO12 ? kin_rows_kernel<1> : kin_rows_kernel<0>;
  hipLaunchKernelGGL(kernel, grid, dim3(KIN_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const double*>(states), mask, n,
                     reinterpret_cast<double*>(out), cfg->use_urdf_inertia, cfg->sim_dt, cfg->gravity);
  return hipGetLastError() == hipSuccess ? 0 : solorl_fail_(SOLORL_ERR_HIP, "solorl_kinematics: kin_rows_kernel launch");
}
