// The DIRECT form of geo_apply_kernel's mapped path (every tap a predicated 4-byte gather from global memory) against the STAGED form
// the library ships (lc2is_amd/csrc/geo.hip: the source box of a block's 32 x 32 output tile is staged in LDS once with 16-byte
// loads when it fits 4096 words per channel, else the block gathers directly), pixels only, B = 32, S = 512.  The direct form is
// the library's own kernel instantiated with a box budget of 0 (geo_apply_kernel<0>), so the arithmetic is the same and the two
// outputs must agree bit for bit; the program checks that and times both.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=fast -I lc2is_amd/csrc -I include tools/probes/geo_staged/geo_staged.hip \
//         -o tools/probes/geo_staged/geo_staged.bin
// Result: README.md next to this file.
#include "../../../lc2is_amd/csrc/geo.hip"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

struct Case { const char* name; double deg, s; };

}  // namespace

int main() {
  const int B = 32, S = 512, rounds = 5, reps = 20;
  const size_t n = (size_t)B * 3 * S * S;
  std::vector<float> h(n);
  unsigned st = 12345u;
  for (auto& v : h) { st = st * 1664525u + 1013904223u; v = (float)(st >> 8) * (1.0f / 8388608.0f) - 1.0f; }
  float *in, *out_d, *out_s;
  int32_t* params;
  const int tiles = (S / GEO_TW) * (S / GEO_TH);
  CHECK(hipMalloc(&in, n * 4)); CHECK(hipMalloc(&out_d, n * 4)); CHECK(hipMalloc(&out_s, n * 4));
  CHECK(hipMalloc(&params, B * GEO_P * 4));
  CHECK(hipMemcpy(in, h.data(), n * 4, hipMemcpyHostToDevice));
  lc2is_geo_config cfg{};
  cfg.warp_thr = 1u << 24; cfg.rotate = 0.3f; cfg.scale_lo = 0.8f; cfg.scale_hi = 1.25f; cfg.ignore_index = -100;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  const Case cases[] = {{"10 degrees, scale 1", 10, 1}, {"45 degrees, scale 0.8", 45, 0.8}, {"90 degrees", 90, 1}, {"scale 0.25", 0, 0.25},
                        {"20 degrees, scale 1.25", 20, 1.25}};
  std::vector<float> a(n), c(n);
  printf("B = %d, S = %d; medians of %d rounds of %d back-to-back launches (device events); TB/s over one read + one write\n", B, S, rounds, reps);
  for (const Case& k : cases) {
    std::vector<int32_t> rows(B * GEO_P, 0);
    const double th = k.deg * M_PI / 180.0, cs = std::cos(th), sn = std::sin(th);
    for (int b = 0; b < B; ++b) {
      int32_t* r = &rows[b * GEO_P];
      r[0] = LC2IS_GEO_WARP;
      r[1] = (int)std::lrint(cs / k.s * 65536); r[2] = (int)std::lrint(-sn / k.s * 65536);
      r[3] = (int)std::lrint(sn / k.s * 65536); r[4] = (int)std::lrint(cs / k.s * 65536);
      r[5] = (b - 16) * 300; r[6] = (16 - b) * 200;   // a small shift of its own per sample
    }
    CHECK(hipMemcpy(params, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
    auto direct = [&] {
      hipLaunchKernelGGL(geo_apply_kernel<0>, dim3(tiles, B), dim3(GEO_THREADS), 0, 0, in, (const int64_t*)nullptr, (const float*)nullptr, params,
                         cfg, S, S, tiles, S / GEO_TW, out_d, (int64_t*)nullptr, (float*)nullptr);
      return 0;
    };
    auto staged = [&] { return lc2is_geo_apply(in, nullptr, nullptr, params, &cfg, B, S, S, out_s, nullptr, nullptr, nullptr); };
    direct();
    if (staged() != 0) { printf("lc2is_geo_apply refused\n"); return 1; }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(a.data(), out_d, n * 4, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(c.data(), out_s, n * 4, hipMemcpyDeviceToHost));
    const bool same = std::memcmp(a.data(), c.data(), n * 4) == 0;
    double t[2][8];
    for (int r = 0; r <= rounds; ++r)
      for (int w = 0; w < 2; ++w) {
        CHECK(hipEventRecord(e0, 0));
        for (int i = 0; i < reps; ++i) { if (w) staged(); else direct(); }
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r) t[w][r - 1] = ms * 1e3 / reps;
      }
    for (int w = 0; w < 2; ++w) std::sort(t[w], t[w] + rounds);
    const double bytes = 2.0 * n * 4;
    printf("%-24s direct %8.1f us (%.1f .. %.1f) %5.2f TB/s | staged %8.1f us (%.1f .. %.1f) %5.2f TB/s | bits %s\n", k.name,
           t[0][rounds / 2], t[0][0], t[0][rounds - 1], bytes / t[0][rounds / 2] / 1e6, t[1][rounds / 2], t[1][0], t[1][rounds - 1],
           bytes / t[1][rounds / 2] / 1e6, same ? "equal" : "DIFFER");
    if (!same) return 2;
  }
  return 0;
}
