// solorl_obs_noise and solorl_actuate (include/solorl.h): what stands between the policy and the engine -- uniform noise on the
// observation rows the engine has written, latency and a per-joint gain error on the action rows it is about to read -- gfx950.
// The arithmetic is csrc/channel.hpp, host-and-device functions; this file is the two kernels' thread mappings and the C entry points.
// Neither kernel knows the engine: they work on the caller's [n][D] and [n][A] float arrays and on caller-owned per-env memory.
//
// Both are small and memory-bound: a row is read once and written once, a Philox block (ten rounds of two 32 x 32 -> 64 bit products)
// is all the arithmetic behind four components.  No LDS (the noise kernel's barrier needs none), no scratch, no atomics.
#include <cmath>
#include <cstddef>

#include "channel.hpp"
#include "row_batch.hpp"

namespace {

constexpr int NOISE_THREADS = 256;

// One thread per (row, block of four components): thread t of a workgroup has row t / B of the workgroup's rows and block t % B, so
// consecutive threads work on consecutive 16 bytes of a row and on consecutive rows behind it.  A workgroup takes NOISE_THREADS / B
// whole rows (at least 4: B <= 53) -- a row never spans two workgroups, because all threads of a row read count[row] and one of them
// writes it, with the workgroup's barrier between the reads and that store.
// VEC: D % 4 == 0 and both arrays 16-byte aligned -- one 16-byte load and one 16-byte store per thread; otherwise word by word.
template <bool VEC>
__global__ __launch_bounds__(NOISE_THREADS) void obs_noise_kernel(solo::ChannelKey key, const float* __restrict__ scale, const uint8_t* __restrict__ mask,
                                                                  int n, int D, int B, int rows_per_group, unsigned* count, const float* obs_in,
                                                                  float* obs_out) {
  using namespace solo;
  const int t = threadIdx.x, r = t / B, b = t - r * B;
  const long long row = (long long)blockIdx.x * rows_per_group + r;
  const bool live = r < rows_per_group && row < n && (mask == nullptr || mask[row] != 0);
  unsigned calls = 0;
  if (live) {
    calls = count[row];
    unsigned w[4];
    noise_block(key, key.id0 + row, calls, B, b, w);
    const size_t at = (size_t)row * D + 4 * b;
    if (VEC) {
      const float4 x = *reinterpret_cast<const float4*>(obs_in + at);
      const float s0 = scale[4 * b], s1 = scale[4 * b + 1], s2 = scale[4 * b + 2], s3 = scale[4 * b + 3];
      // in place, a block of four zero scales is not stored; the zero-scale words of a stored block are their input bits
      if (obs_out != obs_in || s0 != 0.0f || s1 != 0.0f || s2 != 0.0f || s3 != 0.0f)
        *reinterpret_cast<float4*>(obs_out + at) = make_float4(noise_component(w[0], s0, x.x), noise_component(w[1], s1, x.y),
                                                               noise_component(w[2], s2, x.z), noise_component(w[3], s3, x.w));
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int c = 4 * b + k;
        if (c < D) {
          const float s = scale[c];
          if (obs_out != obs_in || s != 0.0f) obs_out[at + k] = noise_component(w[k], s, obs_in[at + k]);
        }
      }
    }
  }
  __syncthreads();                                          // every thread of a row has read count[row]
  if (live && b == 0) count[row] = calls + 1u;
}

constexpr int ACT_LANES = 16, ACT_THREADS = 256;            // 16 lanes per env, joint = lane: an env never spans two wavefronts

// Lane j of an env's 16 has joint j (lanes >= act_dim idle): the levels of buf are rows of 12 floats, so neighbouring lanes touch
// neighbouring words.  Every lane loads the three header words; the 16 lanes are part of ONE wavefront, which executes the loads
// before lane 0's stores.  Philox blocks are drawn by the lanes of restarted envs only.
__global__ __launch_bounds__(ACT_THREADS) void actuate_kernel(solo::ActuateParams p, int n, const uint8_t* __restrict__ restart, float* mem,
                                                              const float* actions_in, float* actions_out) {
  using namespace solo;
  const long long i = ((long long)blockIdx.x * ACT_THREADS + threadIdx.x) / ACT_LANES;
  const int j = threadIdx.x & (ACT_LANES - 1);
  if (i >= n) return;
  float* row = mem + (size_t)i * ACT_ROW_WORDS;
  const unsigned e = (unsigned)actuate_word(row, ACT_OFF_EPISODES);
  int latency = actuate_word(row, ACT_OFF_LATENCY), fill = actuate_word(row, ACT_OFF_FILL);
  const bool fresh = (restart != nullptr && restart[i] != 0) || e == 0u;
  const bool joint = j < p.act_dim;
  if (fresh) {
    latency = actuate_latency(p, p.key.id0 + i, e);
    fill = 0;
    if (joint) row[ACT_OFF_GAIN + j] = actuate_gain(p, p.key.id0 + i, e, j);
  }
  if (joint) {
    const int level = actuate_level(latency, fill);
    const size_t at = (size_t)i * p.act_dim + j;
    const float a = actions_in[at];
    const float d = level < 0 ? a : row[level * 12 + j];
    actions_out[at] = actuate_scale(p, row[ACT_OFF_GAIN + j], d);
    for (int k = p.delay_max - 1; k > 0; k--) row[k * 12 + j] = row[(k - 1) * 12 + j];
    if (p.delay_max > 0) row[j] = a;
  }
  if (j == 0) {
    if (fresh) {
      actuate_set_word(row, ACT_OFF_LATENCY, latency);
      actuate_set_word(row, ACT_OFF_EPISODES, (int)(e + 1u));
    }
    actuate_set_word(row, ACT_OFF_FILL, actuate_fill(fill, p.delay_max));
  }
}

solo::ChannelKey make_key(uint64_t seed, int64_t env_id_offset) { return {(unsigned)seed, (unsigned)(seed >> 32), (long long)env_id_offset}; }

}  // namespace

extern "C" int solorl_obs_noise(uint64_t seed, int64_t env_id_offset, const float* scale, const uint8_t* mask, int n, int D, uint32_t* count,
                                const float* obs_in, float* obs_out, int device_id, void* stream) {
  if (!scale || !count || !obs_in || !obs_out) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_obs_noise: null scale, count, obs_in or obs_out");
  if (n < 1) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_obs_noise: n must be >= 1");
  if (D < 1 || D > solo::CHANNEL_MAX_OBS) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_obs_noise: D must be 1..210");
  if (int rc = solo::select_device(device_id)) return rc;
  const int B = solo::noise_blocks(D), rows = NOISE_THREADS / B;
  const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(obs_in) | reinterpret_cast<uintptr_t>(obs_out)) % 16 == 0;
  hipLaunchKernelGGL(vec ? obs_noise_kernel<true> : obs_noise_kernel<false>, dim3((unsigned)((n - 1) / rows + 1)), dim3(NOISE_THREADS), 0, (hipStream_t)stream,
                     make_key(seed, env_id_offset), scale, mask, n, D, B, rows, count, obs_in, obs_out);
  return hipGetLastError() == hipSuccess ? 0 : solorl_fail_(SOLORL_ERR_HIP, "solorl_obs_noise: obs_noise_kernel launch");
}

extern "C" int solorl_actuate(const solorl_actuation* p, int n, const uint8_t* restart, solorl_env_actuator* mem, const float* actions_in,
                              float* actions_out, int device_id, void* stream) {
  static_assert(sizeof(solorl_env_actuator) == solo::ACT_ROW_WORDS * 4 && offsetof(solorl_env_actuator, gain) == solo::ACT_OFF_GAIN * 4 &&
                offsetof(solorl_env_actuator, latency) == solo::ACT_OFF_LATENCY * 4 && offsetof(solorl_env_actuator, fill) == solo::ACT_OFF_FILL * 4 &&
                offsetof(solorl_env_actuator, episodes) == solo::ACT_OFF_EPISODES * 4 && SOLORL_DELAY_MAX == solo::CHANNEL_DELAY_MAX,
                "channel.hpp addresses solorl_env_actuator by word");
  if (!p || !mem || !actions_in || !actions_out) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_actuate: null params, mem, actions_in or actions_out");
  if (n < 1) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_actuate: n must be >= 1");
  if (p->act_dim != 8 && p->act_dim != 12) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_actuate: act_dim must be 8 or 12");
  if (p->delay_min < 0 || p->delay_min > p->delay_max || p->delay_max > SOLORL_DELAY_MAX)
    return solorl_fail_(SOLORL_ERR_INVALID, "solorl_actuate: the delay range must satisfy 0 <= delay_min <= delay_max <= SOLORL_DELAY_MAX");
  if (!std::isfinite(p->gain_range) || p->gain_range < 0.0 || p->gain_range >= 1.0)
    return solorl_fail_(SOLORL_ERR_INVALID, "solorl_actuate: gain_range must be finite and in [0, 1)");
  if (int rc = solo::select_device(device_id)) return rc;
  const solo::ActuateParams P{make_key(p->seed, p->env_id_offset), p->act_dim, p->delay_min, p->delay_max, p->gain_range};
  const long long threads = (long long)n * ACT_LANES;
  hipLaunchKernelGGL(actuate_kernel, dim3((unsigned)((threads - 1) / ACT_THREADS + 1)), dim3(ACT_THREADS), 0, (hipStream_t)stream, P, n, restart,
                     reinterpret_cast<float*>(mem), actions_in, actions_out);
  return hipGetLastError() == hipSuccess ? 0 : solorl_fail_(SOLORL_ERR_HIP, "solorl_actuate: actuate_kernel launch");
}
