// Host-side check of the skipping plan of the Winograd F(4x4,3x3) path (csrc/wino4_math.h, make_geom4_skip): tiles ordered by
// class so that every frequency plane covers one range of rows, and the planes a partial tile never reads for a stored output
// are neither computed, stored nor loaded.  The same inline functions the HIP kernels call, driven by plain loops.
//   (a) wino4_decode is a bijection onto the tiles, the class counts equal a brute-force count, and each plane kind's range
//       holds exactly the tiles that need the plane;
//   (b) with V and M full of NaN: input body, a reference GEMM over each plane's range only, output body — every stored output
//       equals the dense plan's under memcmp, none is NaN (an untouched output keeps its sentinel in both plans);
//   (c) the cost model's item count (wino4_gemm_items) equals the items enumerated plane by plane, for every tile of UOC_W4_TILES.
// Build + run: tests/test_wino4_skip_host.py (hipcc, no GPU needed).  Exit code 0 = every case passed.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../unseenobjectclustering_amd/csrc/wino4_math.h"

using namespace uoc;

static unsigned long long s_rng = 88172645463325252ull;
static float frand() {  // xorshift, uniform in [-1, 1)
  s_rng ^= s_rng << 13;
  s_rng ^= s_rng >> 7;
  s_rng ^= s_rng << 17;
  return (float)((double)(s_rng >> 11) / 9007199254740992.0 * 2.0 - 1.0);
}

#define CHECK(cond, ...)                   \
  do {                                     \
    if (!(cond)) {                         \
      printf("  FAIL %s: ", #cond);        \
      printf(__VA_ARGS__);                 \
      printf("\n");                        \
      return 1;                            \
    }                                      \
  } while (0)

// class of a tile from its first output pixel, by the definition (not by the plan's arithmetic)
static int brute_class(const Wino4Geom &g, int oy, int ox) {
  if (oy >= g.H || ox >= g.W) return W4_EMPTY;
  const bool row4 = oy + 3 * g.d < g.H, col4 = ox + 3 * g.d < g.W;
  return row4 ? (col4 ? W4_FF : W4_FP) : (col4 ? W4_PF : W4_PP);
}

// (a) and (c)
static int check_plan(int G, int B, int H, int W, int d, long want_unused) {
  const Wino4Geom dense = make_geom4(B, H, W, d), geo = make_geom4_skip(B, H, W, d);
  CHECK(geo.NT == dense.NT && geo.TH == dense.TH && geo.TW == dense.TW, "tile counts differ between the plans");
  // every natural tile exactly once
  std::vector<int> seen((size_t)geo.NT, 0), cls((size_t)geo.NT, -1);
  int count[5] = {0, 0, 0, 0, 0};
  for (int tau = 0; tau < geo.NT; ++tau) {
    int b, oy, ox;
    wino4_decode(tau, geo, b, oy, ox);
    CHECK(b >= 0 && b < B && oy >= 0 && ox >= 0, "tile %d decodes to b=%d oy=%d ox=%d", tau, b, oy, ox);
    const int py = oy % d, ty = oy / d / 4, px = ox % d, tx = ox / d / 4;
    CHECK((oy / d) % 4 == 0 && (ox / d) % 4 == 0 && ty < geo.TH && tx < geo.TW, "tile %d: (%d, %d) is no tile origin", tau, oy, ox);
    const int nat = (((b * d + py) * d + px) * geo.TH + ty) * geo.TW + tx;
    CHECK(!seen[nat], "tile %d decodes to a tile seen before (b=%d oy=%d ox=%d)", tau, b, oy, ox);
    seen[nat] = 1;
    const int c = brute_class(geo, oy, ox);
    cls[tau] = c;
    ++count[c];
    // class-major order and the class the bodies act on
    const int by_range = tau < geo.end[0] ? W4_PF : tau < geo.end[1] ? W4_FF : tau < geo.end[2] ? W4_FP : tau < geo.end[3] ? W4_PP : W4_EMPTY;
    CHECK(c == by_range, "tile %d (oy=%d ox=%d) has class %d but lies in the range of class %d", tau, oy, ox, c, by_range);
    if (c != W4_EMPTY) {
      bool row4, col4;
      wino4_tile_class(tau, geo, row4, col4);
      CHECK(row4 == (c == W4_FF || c == W4_FP) && col4 == (c == W4_FF || c == W4_PF), "tile %d: wino4_tile_class disagrees", tau);
    }
  }
  for (int c = 0; c < 5; ++c) CHECK(count[c] == geo.n[c], "class %d: %d tiles by brute force, %d in the geometry", c, count[c], geo.n[c]);
  // each plane's range holds exactly the tiles that need it
  const Wino4Rows rows = wino4_rows(geo);
  long unused = 0, pairs = 0;
  for (int xi = 0; xi < 36; ++xi) {
    int lo, hi;
    wino4_plane_rows(rows, xi, lo, hi);
    CHECK(0 <= lo && lo <= hi && hi <= geo.NT, "plane %d: range [%d, %d)", xi, lo, hi);
    const int i = xi / 6, j = xi % 6;
    for (int tau = 0; tau < geo.NT; ++tau) {
      const int c = cls[tau];
      const bool needs = c != W4_EMPTY && (i < 5 || c == W4_FF || c == W4_FP) && (j < 5 || c == W4_FF || c == W4_PF);
      CHECK(needs == (tau >= lo && tau < hi), "plane %d, tile %d (class %d): needed %d, range [%d, %d)", xi, tau, c, (int)needs, lo, hi);
      unused += !needs;
    }
    pairs += hi - lo;
  }
  CHECK(pairs == wino4_plane_pairs(rows), "wino4_plane_pairs %ld, enumerated %ld", wino4_plane_pairs(rows), pairs);
  CHECK((long)G * unused == want_unused, "unused (plane, tile) pairs: %ld, expected %ld of %ld", (long)G * unused, want_unused, (long)G * 36 * geo.NT);
  // the dense plan: every plane covers every tile
  const Wino4Rows drows = wino4_rows(dense);
  for (int xi = 0; xi < 36; ++xi) {
    int lo, hi;
    wino4_plane_rows(drows, xi, lo, hi);
    CHECK(lo == 0 && hi == dense.NT, "dense plan, plane %d: range [%d, %d)", xi, lo, hi);
  }
  CHECK(wino4_plane_pairs(drows) == 36l * dense.NT, "dense plan: pairs");
  // (c) items of the plane GEMM, plane by plane, against the cost model's count
  const int tiles[][2] = {
#define X(A, Bn) {A, Bn},
      UOC_W4_TILES(X)
#undef X
  };
  for (const auto &t : tiles)
    for (int ntiles = 1; ntiles <= 8; ntiles *= 2)
      for (int plan = 0; plan < 2; ++plan) {
        const Wino4Rows &r = plan ? drows : rows;
        long items = 0;
        for (int plane = 0; plane < 36 * G; ++plane) {
          int lo, hi;
          wino4_plane_rows(r, plane % 36, lo, hi);
          for (int m0 = lo; m0 < hi; m0 += t[0]) items += ntiles;
        }
        CHECK(items == wino4_gemm_items(r, G, t[0], ntiles), "tile %dx%d, %d n-tiles, plan %d: %ld items enumerated, model %ld", t[0],
              t[1], ntiles, plan, items, wino4_gemm_items(r, G, t[0], ntiles));
        if (plan) CHECK(items == (long)36 * G * ((dense.NT + t[0] - 1) / t[0]) * ntiles, "dense plan: items");
      }
  return 0;
}

// (b): one layer through both plans
template <int VEC>
static int check_layer(int G, int B, int H, int W, int d, int Cin, int Cout, bool use_res, int relu) {
  std::vector<float> in((size_t)G * B * H * W * Cin), w((size_t)G * 9 * Cout * Cin), bias((size_t)G * Cout), res((size_t)G * B * H * W * Cout);
  for (auto &v : in) v = frand();
  for (auto &v : w) v = frand() / sqrtf(9.f * Cin);
  for (auto &v : bias) v = frand();
  for (auto &v : res) v = frand();
  std::vector<float> U((size_t)G * 36 * Cout * Cin);
  for (int g = 0; g < G; ++g)
    for (int co = 0; co < Cout; ++co)
      for (int ci = 0; ci < Cin; ++ci) wino4_weight_body(w.data(), U.data(), G, Cout, Cin, g, co, ci);
  std::vector<float> out[2];
  for (int plan = 0; plan < 2; ++plan) {   // 0: dense, 1: skipping
    const Wino4Geom geo = plan ? make_geom4_skip(B, H, W, d) : make_geom4(B, H, W, d);
    const Wino4Rows rows = wino4_rows(geo);
    std::vector<float> V((size_t)G * 36 * geo.NT * Cin, NAN), M((size_t)G * 36 * geo.NT * Cout, NAN);
    out[plan].assign((size_t)G * B * H * W * Cout, -1e30f);
    for (int g = 0; g < G; ++g)
      for (int tau = 0; tau < geo.NT; ++tau)
        for (int cv = 0; cv < Cin / VEC; ++cv) wino4_input_body<VEC>(in.data(), V.data(), geo, Cin, g, tau, cv);
    for (int gx = 0; gx < G * 36; ++gx) {
      int lo, hi;
      wino4_plane_rows(rows, gx % 36, lo, hi);
      for (int tau = lo; tau < hi; ++tau)
        for (int co = 0; co < Cout; ++co) {
          float acc = 0.f;
          const float *v = &V[((size_t)gx * geo.NT + tau) * Cin], *u = &U[((size_t)gx * Cout + co) * Cin];
          for (int ci = 0; ci < Cin; ++ci) acc = fmaf(v[ci], u[ci], acc);
          M[((size_t)gx * geo.NT + tau) * Cout + co] = acc;
        }
    }
    for (int g = 0; g < G; ++g)
      for (int tau = 0; tau < geo.NT; ++tau)
        for (int cv = 0; cv < Cout / VEC; ++cv)
          wino4_output_body<VEC>(M.data(), bias.data(), use_res ? res.data() : nullptr, out[plan].data(), geo, Cout, relu, g, tau, cv);
    for (size_t i = 0; i < out[plan].size(); ++i) {
      CHECK(!isnan(out[plan][i]), "plan %d: output %zu is NaN", plan, i);
      CHECK(out[plan][i] != -1e30f, "plan %d: output %zu was never stored", plan, i);
    }
  }
  CHECK(memcmp(out[0].data(), out[1].data(), out[0].size() * sizeof(float)) == 0, "the skipping plan's outputs differ from the dense plan's");
  return 0;
}

static int run_case(int G, int B, int H, int W, int d, long want_unused) {
  int bad = check_plan(G, B, H, W, d, want_unused);
  bad += check_layer<4>(G, B, H, W, d, 8, 8, true, 1);
  bad += check_layer<1>(G, B, H, W, d, 4, 4, false, 0);
  printf("G%d B%d %dx%d d%d: %ld unused pairs %s\n", G, B, H, W, d, want_unused, bad ? "FAIL" : "ok");
  return bad;
}

int main() {
  int bad = 0;
  bad += run_case(1, 2, 28, 28, 4, 736);    // stage-2 layer4: 7x7 phase images
  bad += run_case(2, 1, 28, 28, 2, 376);    // stage-2 layer3: 14x14 phase images
  bad += run_case(1, 1, 60, 80, 4, 480);    // stage-1 layer4
  bad += run_case(1, 1, 60, 80, 2, 240);    // stage-1 layer3
  bad += run_case(1, 1, 7, 7, 1, 23);       // one tile of each class
  bad += run_case(1, 1, 8, 8, 1, 0);        // full tiles only
  bad += run_case(1, 1, 56, 56, 1, 0);
  bad += run_case(1, 1, 29, 31, 4, 189);    // ragged phases
  bad += run_case(1, 1, 33, 5, 4, 668);     // ragged, 12 of 48 tiles without a valid output
  bad += run_case(1, 1, 3, 5, 4, 276);      // image smaller than the dilation
  return bad ? 1 : 0;
}
