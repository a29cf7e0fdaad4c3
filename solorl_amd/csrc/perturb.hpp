// perturb.hpp -- the draws of solorl_perturb (include/solorl.h, "Draws"): Philox block -> countdown and kick components.
//
// Plain functions of integers and doubles, host and device alike: perturb_kernel (solorl_hip.hip) calls them per env, solorl_set_perturbation
// calls perturb_first_countdown on the host, and tests/host/perturb_main.cpp compiles this file alone with the host compiler.  Nothing here
// touches the engine's state; the step kernels do not include it.
#ifndef SOLORL_PERTURB_HPP
#define SOLORL_PERTURB_HPP

#if defined(__HIPCC__)
#define PERTURB_HD __host__ __device__ inline
#else
#define PERTURB_HD inline
#endif

namespace solo {

// last counter word of the kicks' Philox stream (the step kernels use 1: goal, 2: settle count of a reset, 3: treadmill side)
constexpr unsigned PERTURB_STREAM = 4u;

struct PerturbParams {
  unsigned seed_lo, seed_hi;     // the handle's seed: the key
  long long id0;                 // env_id_offset: gid = id0 + env id
  int interval_min;
  unsigned span;                 // interval_max - interval_min + 1
  double max_vel[6];             // lin x y z, ang x y z
};

// Philox-4x32-10, the generator of the env's own stream (solorl_hip.hip `philox`, the oracle's oracle_philox)
PERTURB_HD void perturb_philox(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned (&out)[4]) {
  for (int r = 0; r < 10; r++) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// block `block` of env gid's kick stream: counter (gid_lo, gid_hi, block, PERTURB_STREAM)
PERTURB_HD void perturb_block(const PerturbParams& p, long long gid, unsigned block, unsigned (&out)[4]) {
  perturb_philox(p.seed_lo, p.seed_hi, (unsigned)gid, (unsigned)((unsigned long long)gid >> 32), block, PERTURB_STREAM, out);
}

PERTURB_HD int perturb_countdown(const PerturbParams& p, unsigned word) { return p.interval_min + (int)(word % p.span); }

// (2u - 1) max with u = (word >> 8) 2^-24: 2u - 1 is exact, the product rounds once.  max == 0: exactly +0.0, and the caller writes nothing
PERTURB_HD double perturb_component(unsigned word, double max) {
  if (max == 0.0) return 0.0;
  const double u = (double)(word >> 8) * (1.0 / 16777216.0);
  return (2.0 * u - 1.0) * max;
}

// block 0, word 0
PERTURB_HD int perturb_first_countdown(const PerturbParams& p, long long gid) {
  unsigned r[4];
  perturb_block(p, gid, 0u, r);
  return perturb_countdown(p, r[0]);
}

// kick j of env gid (blocks 1 + 2j and 2 + 2j) -> kick[6], returns the countdown to kick j + 1
PERTURB_HD int perturb_kick(const PerturbParams& p, long long gid, unsigned j, double (&kick)[6]) {
  unsigned a[4], b[4];
  perturb_block(p, gid, 1u + 2u * j, a);
  perturb_block(p, gid, 2u + 2u * j, b);
  for (int k = 0; k < 3; k++) { kick[k] = perturb_component(a[k], p.max_vel[k]); kick[3 + k] = perturb_component(b[k], p.max_vel[3 + k]); }
  return perturb_countdown(p, a[3]);
}

}  // namespace solo
#endif  // SOLORL_PERTURB_HPP
