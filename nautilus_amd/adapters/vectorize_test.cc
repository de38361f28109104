// vectorize_test.cc -- drives VectorizeMap (vectorize_hip.h) on clouds and poses the Python test wrote, for
// tests/test_vectorize_adapter.py.
//   vectorize_test <dir>: reads  clouds.bin (int32 n, n int32 point counts, then every cloud's points as float pairs) and
//                                poses.f64 (n x 3 doubles)
//                         writes lines.f32 (the segments, 4 floats each), stats.i32 (8 int32) and map.txt (io::WriteMapLines)
#include <cstdio>
#include <string>
#include <vector>

#include "vectorize_hip.h"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const std::string dir = std::string(argv[1]) + "/";
  std::vector<std::vector<nautilus_hip::Vec2f>> clouds;
  std::vector<std::array<double, 3>> poses;
  {
    FILE *f = fopen((dir + "clouds.bin").c_str(), "rb");
    int32_t n = 0;
    if (!f || fread(&n, sizeof(n), 1, f) != 1 || n < 0) return 3;
    std::vector<int32_t> counts((size_t)n);
    if (n && fread(counts.data(), sizeof(int32_t), (size_t)n, f) != (size_t)n) return 3;
    for (int32_t c : counts) {
      std::vector<float> xy(2 * (size_t)c);
      if (c && fread(xy.data(), sizeof(float), xy.size(), f) != xy.size()) return 3;
      std::vector<nautilus_hip::Vec2f> cloud;
      for (int32_t p = 0; p < c; p++) cloud.push_back(nautilus_hip::Vec2f(xy[2 * p], xy[2 * p + 1]));
      clouds.push_back(cloud);
    }
    fclose(f);
    poses.resize((size_t)n);
    f = fopen((dir + "poses.f64").c_str(), "rb");
    if (!f || (n && fread(poses.data(), 3 * sizeof(double), (size_t)n, f) != (size_t)n)) return 3;
    fclose(f);
  }
  try {
    int32_t stats[8];
    const nhip_vectorize_spec_t spec = nautilus_hip::VectorizeSpec(poses, 30.0);
    const std::vector<nautilus_hip::LineSegment> lines = nautilus_hip::VectorizeMap(clouds, poses, spec, stats);
    FILE *f = fopen((dir + "lines.f32").c_str(), "wb");
    if (!f || (!lines.empty() && fwrite(lines.data(), sizeof(nautilus_hip::LineSegment), lines.size(), f) != lines.size())) return 4;
    fclose(f);
    f = fopen((dir + "stats.i32").c_str(), "wb");
    if (!f || fwrite(stats, sizeof(int32_t), 8, f) != 8) return 4;
    fclose(f);
    if (!nautilus_hip::io::WriteMapLines(dir + "map.txt", lines)) return 4;
    printf("VECTORIZE_OK %zu scans %zu segments\n", clouds.size(), lines.size());
  } catch (const std::exception &e) {
    fprintf(stderr, "vectorize_test: %s\n", e.what());
    return 1;
  }
  return 0;
}
