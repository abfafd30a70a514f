// Object relations of a frame: contact, occlusion and pick order (include/uoc_hip.h, uoc_relations).
// From the label map and the z plane of a frame: the 128x128 tables border / touch / front over the pairs of
// neighbouring pixels that carry different ids, and per id the record uoc_relation_object.  Integers only.
//
// Two memsets (d_pairs, the workspace) and two launches:
//   pair_kernel    grid (pixel chunks of SPAN, frames), 1024 threads.  A lane owns one pixel per turn and visits the
//                  pairs towards its 2 or 4 forward neighbours, read straight from global memory (the neighbour of a
//                  pixel at a row end or a chunk end is just another raster index of the frame: no halo).  A wave whose
//                  lanes all see their own id in every neighbour skips the depth loads and the table work.  The other
//                  pairs become events on ONE table of 128x128 words in LDS, each distinct event added once per wave
//                  (for_each_wave_key of common.h), and every non-zero word leaves the block as
//                  integer atomicAdds: integer adds commute, so the tables do not depend on the order.
//   derive_kernel  one block per frame: row sums, the occlusion masks (128 x 128 bits), the peeling by one wave (two
//                  ids per lane, so a round costs two ballots and no barrier), the rank by counting, the records.
//
// The LDS table.  Word [a][b], a != b, packs two 16-bit counters: the low half counts front[a][b]; the high half counts
// border{a,b} when a < b and touch{a,b} when a > b (both tables are symmetric, so one triangle each is enough).  The
// diagonal word [a][a], which no pair uses, counts the pixels of id a (low half) and those on the image edge (high half).
// Bound of every counter: a block owns SPAN = 8192 pixels; a pixel owns at most 4 pairs (connectivity 8); a pair adds
// at most 1 to one border counter and at most 1 to one touch OR one front counter.  So a border, touch or front counter
// of a block is at most 4 * 8192 = 32768 and a pixel or edge counter at most 8192, all below 65536: no half carries
// into its neighbour (the worst case is a checkerboard of two ids at connectivity 8, where every pair of the block meets
// in one cell).  Across blocks the sums are int32 in global memory: a table entry is at most the number of pairs of a
// frame, below 4 * H*W < 2^31 for H*W < 2^29, and so is a row sum of border.
#include "labelmap.h"
#include "prof.h"

#include <limits.h>

namespace uoc {
namespace {

constexpr int TAB = NUM_IDS * NUM_IDS;
constexpr int PAIR_THREADS = 1024;
constexpr int SPAN = 8192;                // pixels per pair block: 4 * SPAN < 65536, see above
constexpr int TURNS = SPAN / PAIR_THREADS;
constexpr int HI = 1 << 14;               // event code: table word | HI when the event counts in the word's high half
constexpr int CNT_WORDS = 2 * NUM_IDS;    // workspace per frame: pixels[128], edge[128]
constexpr int DERIVE_THREADS = 1024;
constexpr int MAX_PIXELS = (1 << 29) - 1;

static_assert(4 * SPAN < 65536, "a 16-bit counter of a pair block must not wrap");
static_assert(sizeof(uoc_relation_object) == 11 * sizeof(int32_t), "uoc_relation_object is eleven int32");

// One distinct event per loop turn: the wave's lanes holding it are counted with one ballot and added once.
__device__ __forceinline__ void wave_add_events(unsigned *__restrict__ s_tab, int code, int lane) {
  for_each_wave_key(code, [&](int c, unsigned long long m, int first) {
    if (lane == first) atomicAdd(&s_tab[c & (TAB - 1)], (unsigned)__popcll(m) << ((c & HI) ? 16 : 0));
  });
}

// ---- 1. pairs ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PAIR_THREADS) void pair_kernel(const int *__restrict__ labels, const float *__restrict__ xyz,
                                                            int H, int W, int n, int ndir, int gap_mm,
                                                            int *__restrict__ pairs, int *__restrict__ cnt) {
  __shared__ unsigned s_tab[TAB];
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y;
  for (int i = tid; i < TAB / 4; i += PAIR_THREADS) reinterpret_cast<uint4 *>(s_tab)[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  const int *L = labels + (size_t)b * n;
  const float *Z = xyz + ((size_t)b * 3 + 2) * n;
  const int base = blockIdx.x * SPAN;     // below n < 2^29
  for (int k = 0; k < TURNS; ++k) {
    const int wbase = base + k * PAIR_THREADS + (tid - lane);   // wave-uniform
    if (wbase >= n) break;
    const int i = wbase + lane;
    const bool act = i < n;
    int a = 0, x = 0, y = 0;
    bool edge = false;
    if (act) {
      y = i / W;
      x = i - y * W;
      a = obj_id(L[i]);
      edge = x == 0 || y == 0 || x == W - 1 || y == H - 1;
    }
    for_each_wave_key(a > 0 ? a : -1, [&](int id, unsigned long long m, int first) {   // pixels and edge pixels of the ids 1..127
      const unsigned long long me = __ballot(a == id && edge);
      if (lane == first) atomicAdd(&s_tab[id * (NUM_IDS + 1)], (unsigned)__popcll(m) + ((unsigned)__popcll(me) << 16));
    });
    // forward neighbours: right, down, down-right, down-left; every index is inside the frame when its flag holds
    const bool right = act && x + 1 < W, down = act && y + 1 < H;
    const int nj[4] = {i + 1, i + W, i + W + 1, i + W - 1};
    const bool in[4] = {right, down, right && down, down && x > 0};
    int nb[4];
    bool any = false;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      nb[d] = (d < ndir && in[d]) ? obj_id(L[nj[d]]) : a;
      any |= nb[d] != a;
    }
    if (!__any(any)) continue;            // the usual case: no lane of the wave has a pair of two ids
    const int zq = any ? depth_mm(Z[i]) : -1;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      if (d >= ndir) break;               // uniform
      int e_border = -1, e_rel = -1;
      if (nb[d] != a) {
        const int lo = min(a, nb[d]), hi = max(a, nb[d]);
        e_border = HI | (lo * NUM_IDS + hi);
        const int zr = depth_mm(Z[nj[d]]);
        if (zq >= 0 && zr >= 0) {
          const int dz = zq - zr;
          if (abs(dz) < gap_mm)
            e_rel = HI | (hi * NUM_IDS + lo);                            // touch
          else
            e_rel = dz < 0 ? a * NUM_IDS + nb[d] : nb[d] * NUM_IDS + a;  // front[near][far]
        }
      }
      wave_add_events(s_tab, e_border, lane);
      wave_add_events(s_tab, e_rel, lane);
    }
  }
  __syncthreads();
  int *P = pairs + (size_t)b * 3 * TAB;
  int *C = cnt + (size_t)b * CNT_WORDS;
  for (int i = tid; i < TAB; i += PAIR_THREADS) {
    const unsigned v = s_tab[i];
    if (!v) continue;
    const int r = i >> 7, c = i & (NUM_IDS - 1), lo = (int)(v & 0xFFFFu), hi = (int)(v >> 16);
    if (r == c) {
      if (lo) atomicAdd(&C[r], lo);
      if (hi) atomicAdd(&C[NUM_IDS + r], hi);
    } else {
      if (lo) atomicAdd(&P[UOC_REL_FRONT * TAB + i], lo);
      if (hi) {
        int *T = P + (r < c ? UOC_REL_BORDER : UOC_REL_TOUCH) * TAB;
        atomicAdd(&T[i], hi);
        atomicAdd(&T[c * NUM_IDS + r], hi);
      }
    }
  }
}

// ---- 2. relations, layers, order ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(DERIVE_THREADS) void derive_kernel(const int *__restrict__ pairs, const int *__restrict__ cnt,
                                                                int min_pairs, uoc_relation_object *__restrict__ objs) {
  __shared__ int s_border[NUM_IDS], s_ntouch[NUM_IDS], s_nbelow[NUM_IDS], s_layer[NUM_IDS], s_key[NUM_IDS];
  __shared__ unsigned long long s_above[NUM_IDS][2];   // bit a of row b: a occludes b
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const int *P = pairs + (size_t)b * 3 * TAB;
  const int *C = cnt + (size_t)b * CNT_WORDS;
  if (tid < NUM_IDS) {
    s_border[tid] = s_ntouch[tid] = s_nbelow[tid] = s_layer[tid] = 0;
    s_above[tid][0] = s_above[tid][1] = 0ull;
  }
  __syncthreads();
  // the tables are sparse (a frame has a handful of ids), so the LDS atomics below are few
  for (int i = tid; i < TAB; i += DERIVE_THREADS) {
    const int a = i >> 7, c = i & (NUM_IDS - 1);
    const int bo = P[UOC_REL_BORDER * TAB + i];
    if (bo) atomicAdd(&s_border[a], bo);
    if (a >= 1 && c >= 1) {
      if (P[UOC_REL_TOUCH * TAB + i] >= min_pairs) atomicAdd(&s_ntouch[a], 1);
      const int f = P[UOC_REL_FRONT * TAB + i];
      if (f >= min_pairs && f > P[UOC_REL_FRONT * TAB + c * NUM_IDS + a]) {   // a occludes c
        atomicAdd(&s_nbelow[a], 1);
        atomicOr(&s_above[c][a >> 6], 1ull << (a & 63));
      }
    }
  }
  __syncthreads();
  if (tid < 64) {   // peeling: lane owns the ids lane and lane + 64; the layered set is two wave-uniform masks
    const bool p0 = lane >= 1 && C[lane] > 0, p1 = C[lane + 64] > 0;
    const unsigned long long a00 = s_above[lane][0], a01 = s_above[lane][1];
    const unsigned long long a10 = s_above[lane + 64][0], a11 = s_above[lane + 64][1];
    unsigned long long done0 = 0ull, done1 = 0ull;
    int l0 = 0, l1 = 0;
    for (int r = 1;; ++r) {   // every round but the last layers at least one id: at most 128 rounds
      const bool c0 = p0 && l0 == 0 && !(a00 & ~done0) && !(a01 & ~done1);
      const bool c1 = p1 && l1 == 0 && !(a10 & ~done0) && !(a11 & ~done1);
      const unsigned long long n0 = __ballot(c0), n1 = __ballot(c1);
      if (!(n0 | n1)) break;
      if (c0) l0 = r;
      if (c1) l1 = r;
      done0 |= n0;
      done1 |= n1;
    }
    if (p0 && l0 == 0) l0 = -1;
    if (p1 && l1 == 0) l1 = -1;
    s_layer[lane] = l0;
    s_layer[lane + 64] = l1;
    s_key[lane] = p0 ? (l0 < 0 ? NUM_IDS : l0) * NUM_IDS + lane : INT_MAX;
    s_key[lane + 64] = p1 ? (l1 < 0 ? NUM_IDS : l1) * NUM_IDS + lane + 64 : INT_MAX;
  }
  __syncthreads();
  if (tid < NUM_IDS) {
    uoc_relation_object o = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int key = s_key[tid];
    if (key != INT_MAX) {
      int rank = 1;
      for (int j = 0; j < NUM_IDS; ++j) rank += s_key[(j + tid) & (NUM_IDS - 1)] < key;
      o.pixels = C[tid];
      o.edge = C[NUM_IDS + tid];
      o.border = s_border[tid];
      o.border_bg = P[UOC_REL_BORDER * TAB + tid * NUM_IDS];
      o.hidden = P[UOC_REL_FRONT * TAB + tid];
      o.n_touch = s_ntouch[tid];
      o.n_above = (int)(__popcll(s_above[tid][0]) + __popcll(s_above[tid][1]));
      o.n_below = s_nbelow[tid];
      o.layer = s_layer[tid];
      o.free = o.n_above == 0 && o.hidden < min_pairs && o.edge == 0;
      o.order = rank;
    }
    objs[(size_t)b * NUM_IDS + tid] = o;
  }
}

bool shape_ok(int B, int H, int W) {
  return B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= MAX_PIXELS;
}

}  // namespace
}  // namespace uoc

using namespace uoc;

extern "C" {

size_t uoc_relations_workspace_bytes(int B, int H, int W) {
  if (!shape_ok(B, H, W)) return 0;
  return (size_t)B * CNT_WORDS * sizeof(int32_t);
}

int uoc_relations(const int32_t *d_labels, const float *d_xyz, int B, int H, int W, int connectivity, int gap_mm,
                  int min_pairs, int32_t *d_pairs, uoc_relation_object *d_objs, void *d_ws, size_t ws_bytes, void *stream) {
  UOC_REQUIRE(d_labels && d_xyz && d_pairs && d_objs && d_ws, "uoc_relations: null labels / xyz / pairs / objects / workspace");
  UOC_REQUIRE(shape_ok(B, H, W), "uoc_relations: bad shape B=%d H=%d W=%d (B in 1..65535, H*W below 2^29)", B, H, W);
  UOC_REQUIRE(connectivity == 4 || connectivity == 8, "uoc_relations: connectivity = %d is neither 4 nor 8", connectivity);
  UOC_REQUIRE(gap_mm >= 1 && gap_mm <= 65535, "uoc_relations: gap_mm = %d outside [1, 65535]", gap_mm);
  UOC_REQUIRE(min_pairs >= 1, "uoc_relations: min_pairs = %d is below 1", min_pairs);
  UOC_REQUIRE(ws_bytes >= uoc_relations_workspace_bytes(B, H, W), "uoc_relations: workspace %zu < %zu bytes", ws_bytes,
              uoc_relations_workspace_bytes(B, H, W));
  UOC_REQUIRE((((uintptr_t)d_ws | (uintptr_t)d_pairs) & 15) == 0, "uoc_relations: pairs / workspace not 16-byte aligned");
  const int n = H * W;
  hipStream_t st = (hipStream_t)stream;
  int *cnt = (int *)d_ws;
  {
    ProfScope prof(KC_REL_PAIRS, st, 0.0, (double)B * n * 8.0 + (double)B * 3 * TAB * 4.0);
    UOC_HIP_CHECK(hipMemsetAsync(d_pairs, 0, (size_t)B * 3 * TAB * sizeof(int32_t), st));
    UOC_HIP_CHECK(hipMemsetAsync(d_ws, 0, (size_t)B * CNT_WORDS * sizeof(int32_t), st));
    hipLaunchKernelGGL(pair_kernel, dim3((n + SPAN - 1) / SPAN, B), dim3(PAIR_THREADS), 0, st, d_labels, d_xyz, H, W, n,
                       connectivity == 8 ? 4 : 2, gap_mm, d_pairs, cnt);
  }
  {
    ProfScope prof(KC_REL_DERIVE, st, 0.0, (double)B * 3 * TAB * 4.0);
    hipLaunchKernelGGL(derive_kernel, dim3(B), dim3(DERIVE_THREADS), 0, st, d_pairs, cnt, min_pairs, d_objs);
  }
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

}  // extern "C"
