// normals_test.cc -- drives the NormalComputation drop-in on clouds the Python test wrote, for
// tests/test_normals_adapter_gpu.py.
//   normals_test <dir>: reads  clouds.bin (int32 n, n int32 point counts, then every cloud's points as float pairs)
//                       writes single.f32 (GetNormals, one call per cloud) and batch.f32 (GetNormalsBatch, one call): the
//                       normals of all clouds as float pairs, in cloud order
#include <cstdio>
#include <string>
#include <vector>

#include "normal_computation_hip.h"

namespace NC = nautilus::NormalComputation;

static bool write_normals(const std::string &path, const std::vector<std::vector<NC::Vector2f>> &normals) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return false;
  for (const auto &cloud : normals)
    for (const NC::Vector2f &n : cloud) {
      const float v[2] = {n(0), n(1)};
      if (fwrite(v, sizeof(float), 2, f) != 2) return false;
    }
  return fclose(f) == 0;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const std::string dir = std::string(argv[1]) + "/";
  std::vector<std::vector<NC::Vector2f>> clouds;
  {
    FILE *f = fopen((dir + "clouds.bin").c_str(), "rb");
    int32_t n = 0;
    if (!f || fread(&n, sizeof(n), 1, f) != 1 || n < 0) return 3;
    std::vector<int32_t> counts((size_t)n);
    if (n && fread(counts.data(), sizeof(int32_t), (size_t)n, f) != (size_t)n) return 3;
    for (int32_t c : counts) {
      std::vector<float> xy(2 * (size_t)c);
      if (c && fread(xy.data(), sizeof(float), xy.size(), f) != xy.size()) return 3;
      std::vector<NC::Vector2f> cloud;
      for (int32_t p = 0; p < c; p++) cloud.push_back(NC::Vector2f(xy[2 * p], xy[2 * p + 1]));
      clouds.push_back(cloud);
    }
    fclose(f);
  }
  try {
    std::vector<std::vector<NC::Vector2f>> single;
    for (const auto &cloud : clouds) single.push_back(NC::GetNormals(cloud));
    if (!write_normals(dir + "single.f32", single)) return 4;
    if (!write_normals(dir + "batch.f32", NC::GetNormalsBatch(clouds))) return 4;
  } catch (const std::exception &e) {
    fprintf(stderr, "normals_test: %s\n", e.what());
    return 1;
  }
  printf("NORMALS_OK %zu clouds\n", clouds.size());
  return 0;
}
