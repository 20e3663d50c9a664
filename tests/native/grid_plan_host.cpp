// host build of the grid resampler's geometry (banet_amd/csrc/grid_plan.hpp) for tests/test_dense_prep_cpu.py
#include "../../banet_amd/csrc/grid_plan.hpp"
extern "C" float banet_test_grid_coord(int j, float s, float o) { return banet::grid_coord(j, s, o); }
// the candidate range of every texel X in [0, W) along one axis with n outputs
extern "C" void banet_test_grid_ranges(int W, int n, float s, float o, int32_t* lo, int32_t* hi) {
  for (int X = 0; X < W; ++X) {
    int a, b;
    banet::grid_candidates(X, n, s, o, &a, &b);
    lo[X] = a;
    hi[X] = b;
  }
}
extern "C" int banet_test_grid_check_axis(int n_out, int n_in, float s, float o) { return banet::grid_check_axis(n_out, n_in, s, o); }
