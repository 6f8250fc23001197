// Stand-alone sanitizer driver for the top-level tree's host code
// (csrc/rt_tlas.h: world_box, box_pass, the tree union, the cursor walk), beside
// tools/sanitize_driver.cpp. CPU only; rt_tlas.h includes nothing of HIP.
//
//   g++ -std=c++20 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       -o tlas_sanitize_driver tools/tlas_sanitize_driver.cpp   (one line), then ./tlas_sanitize_driver
//
// For K = 1 .. 300 leaf boxes on a jittered lattice (every seventh empty) and
// 64 rays each (an eighth with a zero direction component), the walk's
// candidates under a fixed and under a shrinking tFar must be the leaves that
// pass box_pass, in index order, with the output buffer exactly as long as the
// result (a write past it is the sanitizer's to find).
#include <cstdio>
#include <random>
#include <vector>

#include "../triangles-sdf-cpu-raytracing_amd/csrc/rt_tlas.h"

int main() {
  std::mt19937 rng(18);
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  long checked = 0;
  for (int k = 1; k <= 300; ++k) {
    const int P = rtt::leaf_count(k);
    std::vector<rtt::TNode> nd(2 * (size_t)P, rtt::TNode{{0, 0, 0, 0, 0, 0}, {0, 0}});
    for (int i = 0; i < P; ++i) {
      float *b = nd[(size_t)P + i].b;
      rtt::empty_box(b);
      if (i >= k || i % 7 == 3) continue;
      const float x[12] = {0.5f + 0.2f * u(rng), 0.1f * u(rng), 0, 1.5f * (i % 7) - 4, 0, 0.6f, 0.1f * u(rng),
                           1.5f * ((i / 7) % 7) - 4, 0.1f * u(rng), 0, 0.4f, 1.5f * (i / 49) - 4};
      const float ob[6] = {-1, -1, -1, 1, 1, 1};
      rtt::world_box(x, ob, b);
    }
    for (int n = P - 1; n >= 1; --n) rtt::box_union(nd[2 * (size_t)n].b, nd[2 * (size_t)n + 1].b, nd[(size_t)n].b);
    for (int r = 0; r < 64; ++r) {
      const float o[3] = {6 * u(rng), 6 * u(rng), 6 * u(rng)};
      float d[3] = {u(rng), u(rng), u(rng)};
      if (r % 8 == 0) d[r % 3] = 0.0f;
      const float fixed[1] = {100.0f}, shrink[4] = {8.0f, 4.0f, 2.0f, 0.5f};
      for (int s = 0; s < 2; ++s) {
        const float *tfs = s ? shrink : fixed;
        const int ntf = s ? 4 : 1;
        std::vector<int32_t> want;
        for (int i = 0; i < k; ++i)
          if (rtt::box_pass(nd[(size_t)P + i].b, o, d, 0.01f, tfs[(int)want.size() < ntf ? (int)want.size() : ntf - 1]))
            want.push_back(i);
        std::vector<int32_t> got(want.size());
        const int32_t c = rtt::candidates_host(nd.data(), P, o, d, 0.01f, tfs, ntf, got.data(), (int32_t)got.size());
        if (c != (int32_t)want.size() || got != want) {
          std::printf("FAIL: K = %d ray %d shrink %d: %d candidates, %zu expected\n", k, r, s, c, want.size());
          return 1;
        }
        checked += c;
      }
    }
  }
  std::printf("tlas_sanitize_driver ok: %ld candidates checked\n", checked);
  return 0;
}
