// channel_main.cpp -- the arithmetic of solorl_obs_noise and solorl_actuate (solorl_amd/csrc/channel.hpp) compiled by the host compiler,
// for tests/test_channel_host.py and tests/test_channel_gpu.py (tests/channel_util.py writes and reads the text below).
//
// stdin, one case per line (floats as the hex bit patterns of their 32 bits, gain_range as those of its 64):
//   N seed gid count D in_place scale[D] x[D]         one live noise row -> "count_after y[D]"
//   S seed gid count calls D c scale                  `calls` consecutive noise calls on a zero row with one non-zero scale, at
//       component c -> one line, that component's `calls` outputs (the sign and spread test)
//   A seed gid act_dim delay_min delay_max gain_range T flags actions[T][act_dim]
//       T calls for one env over zeroed memory; flags: T characters, '1' restart, '0' no restart, '-' restart == NULL
//       -> T lines "out[act_dim] row[64]": the applied action and the env's memory row after each call
// Buffers are heap blocks of exactly the sizes the functions may touch, so AddressSanitizer sees an access past D or past the row.
// The kernels call the same functions (solorl_channel.hip).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../solorl_amd/csrc/channel.hpp"

static bool read_words(std::vector<float>& v) {
  for (float& f : v) {
    unsigned w;
    if (std::scanf("%x", &w) != 1) return false;
    std::memcpy(&f, &w, 4);
  }
  return true;
}
static void print_words(const float* p, int n) {
  for (int k = 0; k < n; k++) { unsigned w; std::memcpy(&w, p + k, 4); std::printf("%s%08x", k ? " " : "", w); }
}

int main() {
  char kind;
  int cases = 0;
  while (std::scanf(" %c", &kind) == 1) {
    unsigned long long seed;
    long long gid;
    if (std::scanf("%llu %lld", &seed, &gid) != 2) return 3;
    const solo::ChannelKey key{(unsigned)seed, (unsigned)(seed >> 32), 0};
    if (kind == 'N') {
      unsigned count;
      int D, in_place;
      if (std::scanf("%u %d %d", &count, &D, &in_place) != 3 || D < 1 || D > solo::CHANNEL_MAX_OBS) return 3;
      std::vector<float> scale(D), x(D), y(D);
      if (!read_words(scale) || !read_words(x)) return 3;
      float* out = in_place ? x.data() : y.data();
      solo::channel_noise_row(key, gid, scale.data(), D, &count, x.data(), out);
      std::printf("%u ", count);
      print_words(out, D);
      std::printf("\n");
    } else if (kind == 'S') {
      unsigned count, sbits;
      int D, c, calls;
      if (std::scanf("%u %d %d %d %x", &count, &calls, &D, &c, &sbits) != 5 || D < 1 || D > solo::CHANNEL_MAX_OBS || c < 0 || c >= D) return 3;
      std::vector<float> scale(D, 0.0f), x(D, 0.0f), y(D);
      std::memcpy(&scale[c], &sbits, 4);
      for (int k = 0; k < calls; k++) {
        solo::channel_noise_row(key, gid, scale.data(), D, &count, x.data(), y.data());
        print_words(y.data() + c, 1);
        std::printf(" ");
      }
      std::printf("\n");
    } else if (kind == 'A') {
      solo::ActuateParams p{key, 0, 0, 0, 0.0};
      unsigned long long rbits;
      int T;
      char flags[64];
      if (std::scanf("%d %d %d %llx %d %63s", &p.act_dim, &p.delay_min, &p.delay_max, &rbits, &T, flags) != 6) return 3;
      if ((p.act_dim != 8 && p.act_dim != 12) || T < 1 || (int)std::strlen(flags) != T) return 3;
      std::memcpy(&p.gain_range, &rbits, 8);
      std::vector<float> actions((size_t)T * p.act_dim), row(solo::ACT_ROW_WORDS, 0.0f), out(p.act_dim);
      if (!read_words(actions)) return 3;
      for (int t = 0; t < T; t++) {
        solo::channel_actuate_row(p, gid, flags[t] == '1', row.data(), actions.data() + (size_t)t * p.act_dim, out.data());
        print_words(out.data(), p.act_dim);
        std::printf(" ");
        print_words(row.data(), solo::ACT_ROW_WORDS);
        std::printf("\n");
      }
    } else {
      return 3;
    }
    cases++;
  }
  return cases > 0 ? 0 : 2;
}
