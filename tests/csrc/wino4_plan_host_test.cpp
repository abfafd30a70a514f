// Host-side check of the skipping plan of the Winograd F(4x4,3x3) kernels (csrc/wino4_math.h: make_geom4_skip,
// wino4_decode_skip, wino4_tile_class) at the maps the network's smallest inputs give, where the image is smaller than the
// dilation and whole phases are empty; and the transform bodies under that plan against a direct convolution in double.
// Build + run: tests/test_wino4_host.py (hipcc, no GPU needed).  Exit code 0 = every line ok.
#define main wino4_dense_plan_main
#include "wino4_host_test.cpp"
#undef main

// The skipping plan's tile order (make_geom4_skip, wino4_decode_skip): the tiles with work are exactly the tile origins with
// an output inside the image, each once and in the class the kernels assume; the others decode to origins without one.
static int check_plan(int B, int H, int W, int d) {
  const Wino4Geom g = make_geom4_skip(B, H, W, d), dn = make_geom4(B, H, W, d);
  int bad = 0, inside = 0;
  for (int tau = 0; tau < dn.NT; ++tau) {
    int b, oy, ox;
    wino4_decode_dense(tau, dn, b, oy, ox);
    inside += oy < H && ox < W;
  }
  bad += g.end[3] != inside || g.end[3] + g.n[W4_EMPTY] != g.NT || g.NT != dn.NT;
  std::vector<int> seen((size_t)B * H * W, 0);
  for (int tau = 0; tau < g.NT; ++tau) {
    int b = -1, oy = -1, ox = -1;
    wino4_decode_skip(tau, g, b, oy, ox);
    const bool origin = b >= 0 && b < B && oy >= 0 && ox >= 0 && (oy / d) % 4 == 0 && (ox / d) % 4 == 0 &&
                        oy < 4 * d * g.TH && ox < 4 * d * g.TW;
    if (!origin) {
      ++bad;
      continue;
    }
    if (tau >= g.end[3]) {
      bad += oy < H && ox < W;
      continue;
    }
    if (oy >= H || ox >= W) {
      ++bad;
      continue;
    }
    bad += seen[((size_t)b * H + oy) * W + ox]++ != 0;
    bool row4, col4;
    wino4_tile_class(tau, g, row4, col4);
    bad += row4 != (oy + 3 * d < H) || col4 != (ox + 3 * d < W);
  }
  printf("plan B%d %dx%d d%d: %d tiles, %d with work [PF %d FF %d FP %d PP %d] %s\n", B, H, W, d, g.NT, g.end[3], g.n[W4_PF],
         g.n[W4_FF], g.n[W4_FP], g.n[W4_PP], bad ? "FAIL" : "ok");
  return bad ? 1 : 0;
}

int main() {
  int bad = 0;
  // the 1/8 maps of the smallest inputs the network accepts (8x8 .. 16x8), and ragged ones, at the network's dilations
  const int maps[][2] = {{1, 1}, {2, 1}, {1, 2}, {2, 2}, {3, 5}, {5, 7}, {10, 12}, {9, 13}, {4, 4}, {8, 8}, {17, 6}};
  for (const auto &m : maps)
    for (int d = 1; d <= 4; d *= 2)
      for (int B = 1; B <= 3; B += 2) bad += check_plan(B, m[0], m[1], d);
  bad += run_case<4>(1, 2, 1, 1, 8, 8, 4, true, 1, true);       // one pixel: every tap but the centre outside, all tiles partial
  bad += run_case<2>(2, 1, 2, 1, 8, 8, 2, true, 0, true);
  bad += run_case<4>(1, 3, 2, 2, 8, 12, 4, false, 1, true);
  bad += run_case<1>(1, 2, 5, 7, 4, 8, 4, true, 1, true);       // phases of 2x2 / 1x2 / 2x1 / 1x1 pixels
  bad += run_case<2>(1, 1, 13, 9, 4, 8, 2, true, 1, true);      // every class and empty tiles
  return bad ? 1 : 0;
}
