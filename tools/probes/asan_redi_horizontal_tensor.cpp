// Stand-alone caller of the host entry xg_redi_horizontal_tensor for the host sanitizers (CPU only, no GPU, no Python):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -fwrapv -I. \
//       tools/probes/asan_redi_horizontal_tensor.cpp xgcm_amd/csrc/xg_host.cpp -o /tmp/asan_rediuv && /tmp/asan_rediuv
// from the repository root.  Exact-size heap blocks, five shapes, both face positions, five metric forms, the 27 boundary
// triples, tapered and not, both element types; then the bad calls, which must return a status and write nothing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <cmath>
#include "include/xgcm_hip.h"

template <typename R> static R* block(int64_t n, unsigned seed, double lo, double hi) {
  R* p = (R*)malloc((size_t)(n > 0 ? n : 1) * sizeof(R));
  unsigned s = seed * 2654435761u + 12345u;
  for (int64_t i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; p[i] = (R)(lo + (hi - lo) * ((s >> 8) & 0xffff) / 65535.0); }
  return p;
}

template <typename R> static long run(int dtype) {
  long calls = 0;
  const int64_t shapes[5][4] = {{2, 3, 4, 6}, {1, 1, 1, 1}, {2, 1, 5, 3}, {1, 5, 1, 8}, {3, 2, 7, 1}};
  for (int sh = 0; sh < 5; ++sh) {
    const int64_t L = shapes[sh][0], nz = shapes[sh][1], ny = shapes[sh][2], nx = shapes[sh][3], n = L * nz * ny * nx;
    for (int outer = 0; outer < 2; ++outer) {
      const int64_t nf = nz + outer;
      for (int form = 0; form < 5; ++form) {
        R* b = block<R>(n, 7 + sh, -1, 1);
        R *mx = nullptr, *my = nullptr, *mz = nullptr;
        int64_t sx[4] = {0, 0, 0, 0}, sy[4] = {0, 0, 0, 0}, sz[4] = {0, 0, 0, 0};
        if (form == 1) {  // planes and a profile
          mx = block<R>(ny * nx, 1, 1, 2); my = block<R>(ny * nx, 2, 1, 2); mz = block<R>(nf, 3, 1, 2);
          sx[2] = sy[2] = nx; sx[3] = sy[3] = 1; sz[1] = 1;
        } else if (form == 2) {  // volumes
          mx = block<R>(nz * ny * nx, 1, 1, 2); my = block<R>(nz * ny * nx, 2, 1, 2); mz = block<R>(nf * ny * nx, 3, 1, 2);
          sx[1] = sy[1] = sz[1] = ny * nx; sx[2] = sy[2] = sz[2] = nx; sx[3] = sy[3] = sz[3] = 1;
        } else if (form == 3) {  // with the leading dim
          mx = block<R>(L * nz * ny * nx, 1, 1, 2); my = block<R>(L * nz * ny * nx, 2, 1, 2); mz = block<R>(L * nf * ny * nx, 3, 1, 2);
          sx[0] = sy[0] = nz * ny * nx; sz[0] = nf * ny * nx;
          sx[1] = sy[1] = sz[1] = ny * nx; sx[2] = sy[2] = sz[2] = nx; sx[3] = sy[3] = sz[3] = 1;
        } else if (form == 4) {  // each on its own: mz alone, a profile
          mz = block<R>(nf, 3, 1, 2); sz[1] = 1;
        }
        for (int bx = 1; bx <= 3; ++bx) for (int by = 1; by <= 3; ++by) for (int bz = 1; bz <= 3; ++bz) for (int taper = 0; taper < 2; ++taper) {
          R* ou = (R*)malloc((size_t)n * sizeof(R));
          R* ov = (R*)malloc((size_t)n * sizeof(R));
          const int rc = xg_redi_horizontal_tensor(dtype, b, mx, mx ? sx : nullptr, my, my ? sy : nullptr, mz, mz ? sz : nullptr, 1000.0,
                                                   taper ? 4.0 : 0.0, taper, ou, ov, shapes[sh], 4, outer, bx, 1.75, by, -0.625, bz, 0.375, nullptr);
          if (rc != 0) { printf("unexpected status %d\n", rc); exit(1); }
          volatile R sink = ou[n - 1] + ov[0]; (void)sink;
          free(ou); free(ov);
          ++calls;
        }
        free(b); free(mx); free(my); free(mz);
      }
    }
  }
  // the bad calls: a status, nothing written
  const int64_t shape[3] = {2, 3, 4};
  R* b = block<R>(24, 1, -1, 1);
  R* ou = block<R>(24, 2, 5, 5);
  R* ov = block<R>(24, 3, 5, 5);
  R* m = block<R>(24, 4, 1, 2);
  int64_t st[3] = {12, 4, 1};
  int bad = 0;
#define BAD(...) do { if (xg_redi_horizontal_tensor(__VA_ARGS__) >= 0) { printf("bad call %d accepted\n", bad); exit(1); } ++bad; } while (0)
  BAD(99, b, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1, ou, ov, shape, 3, 0, 1, 0.0, 2, 0.0, 3, 0.0, nullptr);
  BAD(dtype, nullptr, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1, ou, ov, shape, 3, 0, 1, 0.0, 2, 0.0, 3, 0.0, nullptr);
  BAD(dtype, b, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1, nullptr, ov, shape, 3, 0, 1, 0.0, 2, 0.0, 3, 0.0, nullptr);
  BAD(dtype, b, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1, ou, nullptr, shape, 3, 0, 1, 0.0, 2, 0.0, 3, 0.0, nullptr);
  BAD(dtype, b, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1, ou, ov, nullptr, 3, 0, 1, 0.0, 2, 0.0, 3, 0.0, nullptr);
  BAD(dtype, b, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1, ou, ov, shape, 2, 0, 1, 0.0, 2, 0.0, 3, 0.0, nullptr);
  BAD(dtype, b, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1, ou, ov, shape, 3, 2, 1, 0.0, 2, 0.0, 3, 0.0, nullptr);
  BAD(dtype, b, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 2, ou, ov, shape, 3, 0, 1, 0.0, 2, 0.0, 3, 0.0, nullptr);
  BAD(dtype, b, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1, ou, ov, shape, 3, 0, 7, 0.0, 2, 0.0, 3, 0.0, nullptr);
  BAD(dtype, b, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1, ou, ov, shape, 3, 0, 1, 0.0, 0, 0.0, 3, 0.0, nullptr);
  BAD(dtype, b, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1, ou, ov, shape, 3, 0, 1, 0.0, 2, 0.0, 4, 0.0, nullptr);
  BAD(dtype, b, m, 0, 0, 0, 0, 0, 1.0, 1.0, 1, ou, ov, shape, 3, 0, 1, 0.0, 2, 0.0, 3, 0.0, nullptr);
  BAD(dtype, b, 0, 0, m, 0, 0, 0, 1.0, 1.0, 1, ou, ov, shape, 3, 0, 1, 0.0, 2, 0.0, 3, 0.0, nullptr);
  BAD(dtype, b, 0, 0, 0, 0, m, 0, 1.0, 1.0, 1, ou, ov, shape, 3, 0, 1, 0.0, 2, 0.0, 3, 0.0, nullptr);
  BAD(dtype, b, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1, ou, ou, shape, 3, 0, 1, 0.0, 2, 0.0, 3, 0.0, nullptr);
  BAD(dtype, b, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1, ou, ou + 23, shape, 3, 0, 1, 0.0, 2, 0.0, 3, 0.0, nullptr);
  const int64_t noz[3] = {0, 3, 4};
  BAD(dtype, b, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1, ou, ov, noz, 3, 0, 1, 0.0, 2, 0.0, 3, 0.0, nullptr);
  for (int i = 0; i < 24; ++i) if (ou[i] != (R)5 || ov[i] != (R)5) { printf("a bad call wrote\n"); exit(1); }
  const int64_t empty[3] = {2, 0, 4};
  if (xg_redi_horizontal_tensor(dtype, b, m, st, 0, 0, 0, 0, 1.0, 1.0, 1, ou, ov, empty, 3, 1, 1, 0.0, 2, 0.0, 3, 0.0, nullptr) != 0) { printf("empty refused\n"); exit(1); }
  free(b); free(ou); free(ov); free(m);
  printf("element type %d: %ld calls, %d bad calls refused\n", dtype, calls, bad);
  return calls;
}

int main() {
  run<double>(XG_T_F64);
  run<float>(XG_T_F32);
  printf("clean\n");
  return 0;
}
