// Running observation / return normalisation on the device: the reference's VecNormalize (agents/running_mean_std.py:73-127) with its
// RunningMeanStd (:11-39), gfx950.
//
// Why they exist: written with torch ops the wrapper is a dozen launches of a few microseconds per control step (mean, var, the Chan
// merge, sqrt, divide, clip, the accumulator and its masked zeroing), host-ordered, and it does not fit the graphed rollout.
//
// State is caller-owned device memory (no handle): stats = mean[D], var[D], count as 2 D + 1 doubles; ret = n doubles.
//
//   norm_tile_moments_kernel   (mean, M2) of every tile of TE envs x D columns of every row, rows and tiles in parallel
//   norm_row_moments_kernel    a row's tiles -> its batch mean and population variance, rows in parallel
//   norm_scan_kernel           the rows-long Chan merge into the statistics (update_mean_var_count_from_moments, :28-39), one thread per
//                              column; keeps a snapshot of the statistics after every row
//   norm_obs_apply_kernel      out = clip((x - mean) / sqrt(var + epsilon)), every row with its own snapshot
//   norm_ret_accum_kernel      ret = ret gamma + r over the rows, one thread per env (the accumulators do not depend on the statistics);
//                              with update == 0 it scales the rewards too and is the whole call
//   norm_rew_apply_kernel      r = clip(r / sqrt(var + epsilon)), every row with its own snapshot
//
// Launch structure: moments -> row moments -> scan -> apply (rewards: accumulate first), a linear chain on the caller's stream whose
// length does not depend on `rows`; update == 0 is the apply kernel (rewards: the accumulate kernel) alone.
//
// Determinism: everything is fp64 and no sum is ordered by the hardware.  A tile is staged in LDS with coalesced loads; thread (g, c)
// of a workgroup sums column c, c + CW, ... over the envs g, g + G, ... in index order, and the G partial sums of a column are combined
// by a halving tree in LDS (G is a power of two); the row kernel combines the tiles the same way.  TE, CW and G depend on D alone, the
// number of tiles on (n, D): the same inputs give the same bits on every run and replay, and one call over R rows the bits of R calls
// over one row (a row's moments never depend on another row, the scan is sequential either way).  No atomics anywhere.
//
// Numerics: a tile's moments are two-pass (mean first, then the squared deviations from it -- the tile sits in LDS, the second pass is
// free), tiles and rows are merged with the count-weighted formulas, so nothing is ever computed as E[x^2] - E[x]^2.
//
// The stats hazard (a kernel that writes the new statistics while others still read the old ones) is closed by construction: the
// statistics are written by norm_scan_kernel only, which is ONE workgroup; each of its threads reads mean[d] / var[d] of its own columns
// before it writes them, every thread reads `count` before a barrier and thread 0 writes it after its own scan.  The apply kernels
// never read `stats` in an updating call: they read the per-row snapshots in scratch, written by a launch that precedes them on the stream.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "row_batch.hpp"            // select_device (and include/solorl.h, solorl_fail_)

namespace {

using solo::select_device;

constexpr int NT = 256;             // threads of every workgroup here
constexpr int MAX_D = 1024;         // columns (LDS: 4 D + D doubles of partial sums beside the tile)
constexpr int TILE_ELEMS = 2048;    // elements of a tile (16 KB as doubles)
constexpr int MAX_ROWS = 65535;     // rows are the grid's y dimension

struct Shape {
  int TE;        // envs per tile
  int nblk;      // tiles per row
  int cwl;       // log2 of CW = the power of two >= min(D, 64): threads side by side on a row of the tile
  size_t part, bm, snap;   // scratch offsets (doubles): tile moments [rows][nblk][2][D], row moments [rows][2][D], snapshots [rows][2 D + 1]
  size_t acc;              // [rows][n] accumulators before their row's zeroing (D == 1 only)
  size_t total;
};

bool shape_of(int rows, int n, int D, Shape* s) {
  if (rows < 1 || n < 1 || D < 1 || D > MAX_D || rows > MAX_ROWS || (long long)n * D > INT_MAX) return false;
  s->TE = TILE_ELEMS / D;
  if (s->TE > 1024) s->TE = 1024;
  s->nblk = (n + s->TE - 1) / s->TE;
  s->cwl = 0;
  while ((1 << s->cwl) < (D < 64 ? D : 64)) s->cwl++;
  s->part = 0;
  s->bm = s->part + (size_t)rows * s->nblk * 2 * D;
  s->snap = s->bm + (size_t)rows * 2 * D;
  s->acc = s->snap + (size_t)rows * (2 * D + 1);
  s->total = s->acc + (D == 1 ? (size_t)rows * n : 0);
  return s->total <= (size_t)INT_MAX;
}

size_t moments_lds(int D, int cwl, int tile_bytes) { return sizeof(double) * ((size_t)(NT >> cwl) * D + D) + tile_bytes; }

// red[g][d] (g < G) -> red[0][d]: halving tree over g, the same pairs in the same order whatever the data
__device__ __forceinline__ void tree_sum(double* red, int D, int G, int CW, int g, int c) {
  for (int s = G >> 1; s > 0; s >>= 1) {
    __syncthreads();
    if (g < s)
      for (int d = c; d < D; d += CW) red[g * D + d] += red[(g + s) * D + d];
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(NT) void norm_tile_moments_kernel(const T* __restrict__ x, double* __restrict__ part, int n, int D, int TE, int cwl) {
  extern __shared__ double smem[];
  const int G = NT >> cwl, CW = 1 << cwl, tid = threadIdx.x;
  double* red = smem;                  // [G][D]
  double* mu = smem + G * D;           // [D]
  T* tile = reinterpret_cast<T*>(mu + D);     // [cnt][D], the tile's rows as they lie in memory
  const int b = blockIdx.x, r = blockIdx.y, nblk = gridDim.x;
  const int e0 = b * TE, cnt = min(TE, n - e0), m = cnt * D;
  const T* src = x + ((size_t)r * n + e0) * D;
  for (int i = tid; i < m; i += NT) tile[i] = src[i];
  __syncthreads();
  const int c = tid & (CW - 1), g = tid >> cwl;
  for (int d = c; d < D; d += CW) {
    double s = 0.0;
    for (int e = g; e < cnt; e += G) s += (double)tile[e * D + d];
    red[g * D + d] = s;
  }
  tree_sum(red, D, G, CW, g, c);
  if (g == 0)
    for (int d = c; d < D; d += CW) mu[d] = red[d] / (double)cnt;
  __syncthreads();
  for (int d = c; d < D; d += CW) {
    const double mean = mu[d];
    double s = 0.0;
    for (int e = g; e < cnt; e += G) { const double v = (double)tile[e * D + d] - mean; s += v * v; }
    red[g * D + d] = s;
  }
  tree_sum(red, D, G, CW, g, c);
  if (g == 0) {
    double* out = part + ((size_t)r * nblk + b) * 2 * D;
    for (int d = c; d < D; d += CW) { out[d] = mu[d]; out[D + d] = red[d]; }
  }
}

__global__ __launch_bounds__(NT) void norm_row_moments_kernel(const double* __restrict__ part, double* __restrict__ bm, int n, int D, int TE, int nblk, int cwl) {
  extern __shared__ double smem[];
  const int G = NT >> cwl, CW = 1 << cwl, tid = threadIdx.x;
  double* red = smem;
  double* mu = smem + G * D;
  const int r = blockIdx.x, c = tid & (CW - 1), g = tid >> cwl;
  const double* p = part + (size_t)r * nblk * 2 * D;
  for (int d = c; d < D; d += CW) {
    double s = 0.0;
    for (int b = g; b < nblk; b += G) s += (double)min(TE, n - b * TE) * p[(size_t)b * 2 * D + d];
    red[g * D + d] = s;
  }
  tree_sum(red, D, G, CW, g, c);
  if (g == 0)
    for (int d = c; d < D; d += CW) mu[d] = red[d] / (double)n;
  __syncthreads();
  for (int d = c; d < D; d += CW) {
    const double mean = mu[d];
    double s = 0.0;
    for (int b = g; b < nblk; b += G) {
      const double v = p[(size_t)b * 2 * D + d] - mean;
      s += p[(size_t)b * 2 * D + D + d] + (double)min(TE, n - b * TE) * (v * v);
    }
    red[g * D + d] = s;
  }
  tree_sum(red, D, G, CW, g, c);
  if (g == 0) {
    double* out = bm + (size_t)r * 2 * D;
    for (int d = c; d < D; d += CW) { out[d] = mu[d]; out[D + d] = red[d] / (double)n; }
  }
}

// ONE workgroup (see "The stats hazard" above)
__global__ __launch_bounds__(NT) void norm_scan_kernel(double* __restrict__ stats, const double* __restrict__ bm, double* __restrict__ snap, int rows, int n, int D) {
  const int tid = threadIdx.x;
  const size_t S = 2 * (size_t)D + 1;
  const double count0 = stats[2 * D], bn = (double)n;
  __syncthreads();
  for (int d = tid; d < D; d += NT) {
    double mean = stats[d], var = stats[D + d], count = count0;
    for (int r = 0; r < rows; r++) {
      const double bmean = bm[(size_t)r * 2 * D + d], bvar = bm[(size_t)r * 2 * D + D + d];
      const double delta = bmean - mean, tot = count + bn;            // running_mean_std.py:29-37, in its order
      mean = mean + delta * bn / tot;
      var = (var * count + bvar * bn + delta * delta * count * bn / tot) / tot;
      count = tot;
      snap[r * S + d] = mean;
      snap[r * S + D + d] = var;
    }
    stats[d] = mean;
    stats[D + d] = var;
  }
  if (tid == 0) {
    double count = count0;
    for (int r = 0; r < rows; r++) { count += bn; snap[r * S + 2 * D] = count; }
    stats[2 * D] = count;
  }
}

__device__ __forceinline__ double clipped(double y, double clip) { return y < -clip ? -clip : (y > clip ? clip : y); }   // (NaN stays NaN, as np.clip)

// st: the statistics of row r are st + r * stride (stride 0: the same for every row)
__global__ __launch_bounds__(NT) void norm_obs_apply_kernel(const float* __restrict__ x, float* __restrict__ out, const double* __restrict__ st, size_t stride,
                                                            int nD, int D, double clip, double eps) {
  const int i = blockIdx.x * NT + threadIdx.x, r = blockIdx.y;
  if (i >= nD) return;
  const int d = i % D;
  const double* s = st + r * stride;
  const size_t k = (size_t)r * nD + i;
  out[k] = (float)clipped(((double)x[k] - s[d]) / sqrt(s[D + d] + eps), clip);
}

template <bool UPDATE>
__global__ __launch_bounds__(NT) void norm_ret_accum_kernel(double* __restrict__ ret, float* __restrict__ rew, const uint8_t* __restrict__ done, double* __restrict__ acc_rows,
                                                            const double* __restrict__ stats, int rows, int n, double gamma, double clip, double eps) {
  const int e = blockIdx.x * NT + threadIdx.x;
  if (e >= n) return;
  double acc = ret[e];
  const double sd = UPDATE ? 1.0 : sqrt(stats[1] + eps);
  for (int t = 0; t < rows; t++) {
    const size_t k = (size_t)t * n + e;
    const float r = rew[k];
    acc = __dadd_rn(__dmul_rn(acc, gamma), (double)r);       // (unfused: the reference's two roundings)
    if (UPDATE) acc_rows[k] = acc;
    else rew[k] = (float)clipped((double)r / sd, clip);
    if (done[k]) acc = 0.0;
  }
  ret[e] = acc;
}

__global__ __launch_bounds__(NT) void norm_rew_apply_kernel(float* __restrict__ rew, const double* __restrict__ snap, int n, double clip, double eps) {
  const int e = blockIdx.x * NT + threadIdx.x, r = blockIdx.y;
  if (e >= n) return;
  const size_t k = (size_t)r * n + e;
  rew[k] = (float)clipped((double)rew[k] / sqrt(snap[(size_t)r * 3 + 1] + eps), clip);
}

// moments of rows x [n][D] values -> the statistics and their per-row snapshots
template <typename T>
int update_stats(double* stats, const T* x, int rows, int n, int D, const Shape& s, double* scratch, hipStream_t st) {
  hipLaunchKernelGGL(norm_tile_moments_kernel<T>, dim3(s.nblk, rows), dim3(NT), moments_lds(D, s.cwl, s.TE * D * (int)sizeof(T)), st, x, scratch + s.part, n, D, s.TE, s.cwl);
  hipLaunchKernelGGL(norm_row_moments_kernel, dim3(rows), dim3(NT), moments_lds(D, s.cwl, 0), st, scratch + s.part, scratch + s.bm, n, D, s.TE, s.nblk, s.cwl);
  hipLaunchKernelGGL(norm_scan_kernel, dim3(1), dim3(NT), 0, st, stats, scratch + s.bm, scratch + s.snap, rows, n, D);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace

extern "C" {

int solorl_norm_scratch_count(int rows, int n, int D) {
  Shape s;
  return shape_of(rows, n, D, &s) ? (int)s.total : 0;
}

int solorl_normalize_obs(double* stats, int rows, int n, int D, const float* obs_in, float* obs_out, int update, double clip, double epsilon,
                         double* scratch, int device_id, void* stream) {
  if (!stats || !obs_in || !obs_out) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_normalize_obs: null array");
  if (rows < 1 || n < 1 || D < 1) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_normalize_obs: rows, n and D must be >= 1");
  Shape s;
  if (!shape_of(rows, n, D, &s)) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_normalize_obs: shape out of range (D <= 1024, rows <= 65535, n D < 2^31, scratch < 2^31 doubles)");
  if (!scratch) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_normalize_obs: null scratch");
  if (int rc = select_device(device_id)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (update && update_stats(stats, obs_in, rows, n, D, s, scratch, st)) return solorl_fail_(SOLORL_ERR_HIP, "solorl_normalize_obs: moments launch");
  const int nD = n * D;
  hipLaunchKernelGGL(norm_obs_apply_kernel, dim3((nD + NT - 1) / NT, rows), dim3(NT), 0, st, obs_in, obs_out, update ? scratch + s.snap : stats,
                     update ? (size_t)(2 * D + 1) : (size_t)0, nD, D, clip, epsilon);
  return hipGetLastError() == hipSuccess ? 0 : solorl_fail_(SOLORL_ERR_HIP, "solorl_normalize_obs: norm_obs_apply_kernel launch");
}

int solorl_normalize_rewards(double* stats, double* ret, int rows, int n, float* rewards, const uint8_t* done, int update, double gamma, double clip,
                             double epsilon, double* scratch, int device_id, void* stream) {
  if (!stats || !ret || !rewards || !done) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_normalize_rewards: null array");
  if (rows < 1 || n < 1) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_normalize_rewards: rows and n must be >= 1");
  Shape s;
  if (!shape_of(rows, n, 1, &s)) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_normalize_rewards: shape out of range (rows <= 65535, scratch < 2^31 doubles)");
  if (!scratch) return solorl_fail_(SOLORL_ERR_INVALID, "solorl_normalize_rewards: null scratch");
  if (int rc = select_device(device_id)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const dim3 envs((n + NT - 1) / NT);
  if (!update) {
    hipLaunchKernelGGL(norm_ret_accum_kernel<false>, envs, dim3(NT), 0, st, ret, rewards, done, (double*)nullptr, stats, rows, n, gamma, clip, epsilon);
    return hipGetLastError() == hipSuccess ? 0 : solorl_fail_(SOLORL_ERR_HIP, "solorl_normalize_rewards: norm_ret_accum_kernel launch");
  }
  hipLaunchKernelGGL(norm_ret_accum_kernel<true>, envs, dim3(NT), 0, st, ret, rewards, done, scratch + s.acc, stats, rows, n, gamma, clip, epsilon);
  if (update_stats(stats, scratch + s.acc, rows, n, 1, s, scratch, st)) return solorl_fail_(SOLORL_ERR_HIP, "solorl_normalize_rewards: moments launch");
  hipLaunchKernelGGL(norm_rew_apply_kernel, dim3(envs.x, rows), dim3(NT), 0, st, rewards, scratch + s.snap, n, clip, epsilon);
  return hipGetLastError() == hipSuccess ? 0 : solorl_fail_(SOLORL_ERR_HIP, "solorl_normalize_rewards: norm_rew_apply_kernel launch");
}

}  // extern "C"
