// tools/vectorize_host_check.cc -- the pure-host entry points of the map vectorisation (tables, pose affines, workspace
// layout, spec validation, endpoints) under AddressSanitizer + UBSan, as a stand-alone program: CPU only, never loaded into
// Python.  Build and run from nautilus_amd/csrc:
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined"
//   for u in nhip_host_vectorize nhip_vectorize nhip_runtime; do hipcc $F -c $u.hip -o /tmp/$u.o; done
//   hipcc $F -I../../include -x hip -c ../../tools/vectorize_host_check.cc -o /tmp/check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/check.o /tmp/nhip_*.o -o /tmp/vectorize_host_check -ldl && /tmp/vectorize_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include "nautilus_hip.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s line %d: %s\n", #c, __LINE__, nhip_last_error()); return 1; } } while (0)
int main() {
  nhip_vectorize_spec_t s;
  CHECK(nhip_vectorize_spec_default(&s) == NHIP_OK);
  CHECK(nhip_vectorize_spec_default(nullptr) == NHIP_ERR_ARG);
  s.width = 96; s.height = 64; s.n_theta = 4; s.min_hits = 1; s.min_votes = 3;
  for (int nt : {2, 3, 360, 1024}) {
    nhip_vectorize_spec_t q = s; q.n_theta = nt;
    std::vector<int32_t> C(nt), S(nt);
    CHECK(nhip_vectorize_tables(&q, C.data(), S.data()) == NHIP_OK);
    CHECK(C[0] == 16384 && S[0] == 0);
  }
  // validation: each bad field
  { nhip_vectorize_layout_t L; nhip_vectorize_spec_t b;
    b = s; b.res = 0; CHECK(nhip_vectorize_workspace_layout(&b, 10, &L) == NHIP_ERR_ARG);
    b = s; b.res = NAN; CHECK(nhip_vectorize_workspace_layout(&b, 10, &L) == NHIP_ERR_ARG);
    b = s; b.width = 0; CHECK(nhip_vectorize_workspace_layout(&b, 10, &L) == NHIP_ERR_ARG);
    b = s; b.height = 16385; CHECK(nhip_vectorize_workspace_layout(&b, 10, &L) == NHIP_ERR_ARG);
    b = s; b.min_hits = 0; CHECK(nhip_vectorize_workspace_layout(&b, 10, &L) == NHIP_ERR_ARG);
    b = s; b.n_theta = 1025; CHECK(nhip_vectorize_workspace_layout(&b, 10, &L) == NHIP_ERR_ARG);
    b = s; b.min_votes = 0; CHECK(nhip_vectorize_workspace_layout(&b, 10, &L) == NHIP_ERR_ARG);
    b = s; b.band = 0.1; CHECK(nhip_vectorize_workspace_layout(&b, 10, &L) == NHIP_ERR_ARG);
    b = s; b.band = INFINITY; CHECK(nhip_vectorize_workspace_layout(&b, 10, &L) == NHIP_ERR_ARG);
    b = s; b.max_gap = -1; CHECK(nhip_vectorize_workspace_layout(&b, 10, &L) == NHIP_ERR_ARG);
    b = s; b.min_length = 0; CHECK(nhip_vectorize_workspace_layout(&b, 10, &L) == NHIP_ERR_ARG);
    b = s; b.max_segments = -1; CHECK(nhip_vectorize_workspace_layout(&b, 10, &L) == NHIP_ERR_ARG);
    CHECK(nhip_vectorize_workspace_layout(&s, -1, &L) == NHIP_ERR_ARG);
    CHECK(nhip_vectorize_workspace_bytes(&b, 10) == -1);
    int32_t st[8];
    CHECK(nhip_vectorize_dev(nullptr, nullptr, nullptr, 0, &b, 1, 1, 1, nullptr, st, nullptr, 0, nullptr) == NHIP_ERR_ARG);
    CHECK(nhip_vectorize(nullptr, nullptr, &b, 1, 1, 1, nullptr, st) == NHIP_ERR_ARG);
  }
  const int geo[6][3] = {{1, 1, 0}, {16384, 1, 200}, {1, 16384, 200}, {7, 5, 35}, {130, 67, 1000}, {16384, 16384, 1 << 26}};
  for (auto &g : geo) {
    nhip_vectorize_spec_t q = s; q.width = g[0]; q.height = g[1]; q.n_theta = 1024;
    nhip_vectorize_layout_t L;
    CHECK(nhip_vectorize_workspace_layout(&q, g[2], &L) == NHIP_OK);
    CHECK(L.counts_offset % 256 == 0 && L.counts_offset < L.cells_offset && L.cells_offset < L.votes_offset && L.votes_offset < L.live_offset && L.live_offset < L.bytes);
    CHECK(nhip_vectorize_workspace_bytes(&q, g[2]) == L.bytes);
    std::printf("%d x %d, %d cells: %lld bytes\n", g[0], g[1], g[2], (long long)L.bytes);
  }
  double poses[9] = {0, 0, 0, 1e-300, -1e300, 3.14159, 3.1, -2.2, 1e6};
  float aff[12];
  CHECK(nhip_map_pose_affines(poses, 3, aff) == NHIP_OK && aff[0] == 1.0f && aff[1] == 0.0f);
  CHECK(nhip_map_pose_affines(nullptr, 0, nullptr) == NHIP_OK);
  // the crafted records of tests/test_vectorize_cpu.py: one_line, tie, diag_neg (a_lo < 0), extreme bins
  const int64_t rec[5][10] = {{2, 116, 57, 86, 30, 735, 600, 20255, 14700, 12000},
                              {0, 116, 101, 120, 20, 400, 290, 8000, 5800, 4870},
                              {3, 67, -11, 45, 40, 3020, 1420, 233350, 112550, 55750},
                              {1, 0, -64, 159, 1, 95, 63, 9025, 5985, 3969},
                              {3, 256, 159, 159, 1, 0, 0, 0, 0, 0}};
  float lines[20];
  CHECK(nhip_vectorize_endpoints(&s, &rec[0][0], 5, lines) == NHIP_OK);
  for (int i = 0; i < 5; i++) std::printf("%g,%g,%g,%g\n", lines[4 * i], lines[4 * i + 1], lines[4 * i + 2], lines[4 * i + 3]);
  CHECK(std::fabs(lines[0] - 1.975f) < 1e-6f && std::fabs(lines[1] - 1.025f) < 1e-6f);
  CHECK(nhip_vectorize_endpoints(&s, nullptr, 0, nullptr) == NHIP_OK);
  int64_t bad[10] = {4, 0, 0, 0, 1, 0, 0, 0, 0, 0};
  CHECK(nhip_vectorize_endpoints(&s, bad, 1, lines) == NHIP_ERR_ARG);  // row outside the table
  bad[0] = -1;
  CHECK(nhip_vectorize_endpoints(&s, bad, 1, lines) == NHIP_ERR_ARG);
  std::printf("sanitiser run clean\n");
  return 0;
}
