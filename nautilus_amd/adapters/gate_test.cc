// gate_test.cc -- drives CorrelativeScanMatcherBatch with and without its score gate on clouds the Python test wrote, for
// tests/test_csm_gate_gpu.py.
//   gate_test <dir>: reads  clouds.txt (n, then per cloud its point count and "x y" lines), pairs.txt (n, then "source
//                    target" lines), rotations.txt (n, then one heading per cloud), params.txt (scanner_range res n_theta nx
//                    ny theta_step min_score); every number as C reads it (hex floats included)
//                    writes ungated.txt and gated.txt: per pair "score tx ty rotation" in hex floats
#include <cstdio>
#include <string>
#include <vector>

#include "CorrelativeScanMatcher.h"

using Batch = CorrelativeScanMatcherBatch;

static bool write_results(const std::string &path, const std::vector<Batch::Result> &res) {
  FILE *f = fopen(path.c_str(), "w");
  if (!f) return false;
  for (const Batch::Result &r : res)
    fprintf(f, "%a %a %a %a\n", r.score, (double)r.translation.x(), (double)r.translation.y(), (double)r.rotation);
  return fclose(f) == 0;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const std::string dir = std::string(argv[1]) + "/";
  std::vector<std::vector<Batch::Vector2f>> clouds;
  std::vector<std::pair<size_t, size_t>> pairs;
  std::vector<double> rotations;
  double scanner_range, res, theta_step, min_score;
  nhip_search_t search = {0, 0, 0, 0, 0.0};
  {
    FILE *f = fopen((dir + "clouds.txt").c_str(), "r");
    int n = 0;
    if (!f || fscanf(f, "%d", &n) != 1) return 3;
    clouds.resize((size_t)n);
    for (auto &c : clouds) {
      int m = 0;
      if (fscanf(f, "%d", &m) != 1) return 3;
      for (int i = 0; i < m; i++) {
        float x, y;
        if (fscanf(f, "%f %f", &x, &y) != 2) return 3;
        c.push_back(Batch::Vector2f(x, y));
      }
    }
    fclose(f);
  }
  {
    FILE *f = fopen((dir + "pairs.txt").c_str(), "r");
    int n = 0;
    if (!f || fscanf(f, "%d", &n) != 1) return 4;
    for (int i = 0; i < n; i++) {
      size_t s, t;
      if (fscanf(f, "%zu %zu", &s, &t) != 2) return 4;
      pairs.emplace_back(s, t);
    }
    fclose(f);
  }
  {
    FILE *f = fopen((dir + "rotations.txt").c_str(), "r");
    int n = 0;
    if (!f || fscanf(f, "%d", &n) != 1) return 5;
    rotations.resize((size_t)n);
    for (double &r : rotations)
      if (fscanf(f, "%lf", &r) != 1) return 5;
    fclose(f);
  }
  {
    FILE *f = fopen((dir + "params.txt").c_str(), "r");
    if (!f || fscanf(f, "%lf %lf %d %d %d %lf %lf", &scanner_range, &res, &search.n_theta, &search.nx, &search.ny, &theta_step,
                     &min_score) != 7)
      return 6;
    fclose(f);
    search.theta_step = theta_step;
  }
  try {
    const Batch plain(scanner_range, res, search);
    const Batch gated(scanner_range, res, search, min_score);
    if (!write_results(dir + "ungated.txt", plain.Match(clouds, pairs, rotations))) return 7;
    if (!write_results(dir + "gated.txt", gated.Match(clouds, pairs, rotations))) return 7;
  } catch (const std::exception &e) {
    fprintf(stderr, "gate_test: %s\n", e.what());
    return 1;
  }
  return 0;
}
