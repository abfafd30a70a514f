// Grasp candidates: a parallel-jaw fit on the table grid (include/uoc_hip.h, uoc_grasp).
// From the state / owner grids of uoc_placement and a host table of A closing directions: for every id 1..127 and every
// candidate (direction k, lateral offset m) how wide the object is along the closing direction and whether both fingers
// land on free table (cand), and the best candidate per id (best).  Integers only.
//
// One memset (the moments in the workspace) and two launches:
//   moments_kernel    grid (chunks of CHUNK cells, frames), 4 waves.  n_a, sum i, sum j per id: the wave adds every
//                     DISTINCT id of its 64 cells once (ballot, popcount and two wave_sums of common.h) to an LDS
//                     table, the block flushes its non-zero words with integer atomics.
//   candidate_kernel  grid (ids 0..127, frames), 4 waves, dynamic LDS.  Block 0 and the block of an absent id zero
//                     their rows and leave.  The others loop over the directions in chunks of KC that fit the class table:
//                       pass 1  a wave owns a line (k, l), its lanes sweep t: the class of the sample, one byte, to LDS;
//                               l in -(M+Hp)..(M+Hp), t in -(R+gap+F)..(R+gap+F): neighbouring m share their lines
//                       pass 2  a thread owns a candidate (k, m): it walks its strip in LDS and writes (code, tlo)
//                     then the key maximum per wave by shuffles, per block by one LDS atomicMax; the thread that holds the
//                     winning key writes the best record (the key is a strict total order over (k, m): one thread).
//
// The grid's constants and the host-side shape checks are grid.h's, the shuffle reductions common.h's.
//
// Determinism: integer adds and maxima commute and the key is a strict total order, so no result depends on the order in
// which lanes, waves or blocks arrive.  Nothing of frame b depends on the other frames of the batch.
#include "grid.h"
#include "prof.h"

namespace uoc {
namespace {

constexpr int SHIFT = 14;  // S = 1 << SHIFT
constexpr int MAX_A = UOC_GRASP_MAX_DIRS, MAX_M = UOC_GRASP_MAX_OFFSETS, MAX_W = UOC_GRASP_MAX_OPEN, MAX_GAP = UOC_GRASP_MAX_GAP,
              MAX_F = UOC_GRASP_MAX_FINGER, MAX_HP = UOC_GRASP_MAX_PAD;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int CHUNK = 8 * THREADS;     // cells per block of the moments pass
constexpr int MOM = 4;                 // words per (frame, id) in the workspace: n, sum i, sum j, 0
constexpr int TABLE_CAP = 48 * 1024;   // bytes of class table per block
enum : unsigned char { C_OWN = 0, C_FREE = 1, C_OTHER = 2, C_OUT = 3, C_UNKNOWN = 4 };

static_assert(SCALE == 1 << SHIFT && (long long)MAX_G * MAX_G * (MAX_G - 1) < INT_MAX, "sum i of one id must fit an int32");
static_assert((2 * (MAX_M + MAX_HP) + 1) * (2 * (2 * MAX_W + MAX_GAP + MAX_F) + 1) <= TABLE_CAP, "one direction must fit the class table");
static_assert((long long)MAX_G * SCALE + (2 * MAX_W + MAX_GAP + MAX_F + MAX_M + MAX_HP) * 2ll * SCALE < INT_MAX, "X, Y must fit an int32");
static_assert(MAX_M < 16 && MAX_W <= 256 && MAX_A <= 256, "the key's fields");

struct Dirs {
  int c[MAX_A][2];  // (Cx, Cy)
};

struct Params {
  int G, A, M, Wmax, gap, F, Hp, unknown_blocks;
  int R, E, T, NLn, KC;  // R = 2 Wmax, E = R + gap + F, T = 2 E + 1 samples per line, NLn lines per direction, KC directions per chunk
};

// ---- 1. moments -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void moments_kernel(const int *__restrict__ state, const int *__restrict__ owner, int G,
                                                          int *__restrict__ mom) {
  __shared__ int s_m[NUM_IDS * 3];
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y;
  const int cells = G * G;
  for (int i = tid; i < NUM_IDS * 3; i += THREADS) s_m[i] = 0;
  __syncthreads();
  const int *St = state + (size_t)b * cells, *Ow = owner + (size_t)b * cells;
#pragma unroll  // as the compiler did unasked while the group loop stood here in full
  for (int r = 0; r < CHUNK / THREADS; ++r) {
    const int base = blockIdx.x * CHUNK + r * THREADS + (tid - lane);
    if (base >= cells) break;  // uniform per wave
    const int idx = base + lane;
    int id = -1, i = 0, j = 0;
    if (idx < cells && St[idx] == 2) {
      const int o = Ow[idx];
      if (obj_id(o)) {
        id = o;
        i = idx / G;
        j = idx - i * G;
      }
    }
    for_each_wave_key(id, [&](int c, unsigned long long m, int first) {  // every lane takes part in the shuffles
      const bool hit = id == c;
      const int si = wave_sum(hit ? i : 0), sj = wave_sum(hit ? j : 0);
      if (lane == first) {
        atomicAdd(&s_m[c * 3], (int)__popcll(m));
        atomicAdd(&s_m[c * 3 + 1], si);
        atomicAdd(&s_m[c * 3 + 2], sj);
      }
    });
  }
  __syncthreads();
  for (int i = tid; i < NUM_IDS * 3; i += THREADS) {
    const int v = s_m[i];
    if (v) atomicAdd(&mom[((size_t)b * NUM_IDS + i / 3) * MOM + i % 3], v);
  }
}

// ---- 2. candidates ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void candidate_kernel(const int *__restrict__ state, const int *__restrict__ owner,
                                                            const int *__restrict__ mom, Dirs d, Params p,
                                                            int *__restrict__ cand, int *__restrict__ best) {
  extern __shared__ unsigned char s_cls[];  // [KC][NLn][T]
  __shared__ unsigned s_key;
  __shared__ int s_nok;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = blockIdx.x, b = blockIdx.y;
  const int G = p.G, A = p.A, M = p.M, Hp = p.Hp, R = p.R, E = p.E, T = p.T, NLn = p.NLn, NM = 2 * p.M + 1;
  int *C = cand + ((size_t)b * NUM_IDS + a) * (size_t)(A * NM * 2);
  int *Bst = best + ((size_t)b * NUM_IDS + a) * 8;
  const int *mo = mom + ((size_t)b * NUM_IDS + a) * MOM;
  const int n = a ? mo[0] : 0;
  if (n == 0) {  // uniform per block
    for (int i = tid; i < A * NM * 2; i += THREADS) C[i] = 0;
    if (tid < 8) Bst[tid] = 0;
    return;
  }
  // the sums are not negative: truncation is floor
  const int ax = (int)(((long long)SCALE * (2ll * mo[1] + n)) / (2ll * n));
  const int ay = (int)(((long long)SCALE * (2ll * mo[2] + n)) / (2ll * n));
  if (tid == 0) {
    s_key = 0u;
    s_nok = 0;
  }
  const int *St = state + (size_t)b * G * G, *Ow = owner + (size_t)b * G * G;
  unsigned my_key = 0u;
  int my_k = 0, my_m = 0, my_tlo = 0, my_w = 0, my_ok = 0;
  for (int k0 = 0; k0 < A; k0 += p.KC) {
    const int kc = min(p.KC, A - k0);
    __syncthreads();  // the previous chunk's pass 2 is done with the table
    const int rows = kc * NLn;
    for (int row = wave; row < rows; row += WAVES) {  // pass 1
      const int kk = row / NLn, l = row - kk * NLn - (M + Hp);
      const int cx = d.c[k0 + kk][0], cy = d.c[k0 + kk][1];
      unsigned char *line = s_cls + row * T;
      for (int ti = lane; ti < T; ti += 64) {
        const int t = ti - E;
        const int i = (ax + t * cx - l * cy) >> SHIFT, j = (ay + t * cy + l * cx) >> SHIFT;  // arithmetic shifts: floor
        unsigned char cls = C_OUT;
        if ((unsigned)i < (unsigned)G && (unsigned)j < (unsigned)G) {
          const int st = St[i * G + j];
          if (st == 2) {
            const int o = Ow[i * G + j];
            cls = o == a ? C_OWN : ((unsigned)(o - 1) < (unsigned)(NUM_IDS - 1) ? C_OTHER : C_UNKNOWN);
          } else {
            cls = (st == 1 || (st == 0 && !p.unknown_blocks)) ? C_FREE : C_UNKNOWN;
          }
        }
        line[ti] = cls;
      }
    }
    __syncthreads();
    for (int c = tid; c < kc * NM; c += THREADS) {  // pass 2
      const int kk = c / NM, mi = c - kk * NM, m = mi - M, k = k0 + kk;
      const unsigned char *strip = s_cls + (kk * NLn + mi) * T + E;  // line l = m - Hp is line mi of the direction; strip[t]
      int tlo = INT_MAX, thi = INT_MIN;
      for (int ln = 0; ln <= 2 * Hp; ++ln) {
        const unsigned char *line = strip + ln * T;
        for (int t = -R; t <= R; ++t)
          if (line[t] == C_OWN) {
            tlo = min(tlo, t);
            thi = max(thi, t);
          }
      }
      int code = -1, w = 0;
      if (thi < tlo) {
        tlo = 0;
      } else if ((w = thi - tlo + 1) > p.Wmax) {
        code = -2;
      } else {
        bool pinched = false, blocked = false;
        const int reach = p.gap + p.F;
        for (int ln = 0; ln <= 2 * Hp; ++ln) {
          const unsigned char *line = strip + ln * T;
          for (int t = tlo; t <= thi; ++t) pinched = pinched || line[t] == C_OTHER || line[t] == C_OUT;
          for (int s = 1; s <= reach; ++s) blocked = blocked || line[tlo - s] != C_FREE || line[thi + s] != C_FREE;
        }
        code = pinched ? -3 : (blocked ? -4 : w);
      }
      C[(k * NM + mi) * 2] = code;
      C[(k * NM + mi) * 2 + 1] = tlo;
      if (code > 0) {
        ++my_ok;
        const unsigned key = 1u + (((unsigned)(M - abs(m)) << 24) | ((unsigned)(p.Wmax - w) << 16) | ((unsigned)(A - 1 - k) << 8) |
                                   (m >= 0 ? 1u : 0u));
        if (key > my_key) {
          my_key = key;
          my_k = k;
          my_m = m;
          my_tlo = tlo;
          my_w = w;
        }
      }
    }
  }
  unsigned wkey = my_key;
  int wok = my_ok;
#pragma unroll
  // Spelled out, not common.h's helpers: the key is unsigned and wave_max is a signed reduction.  This loop is the code
  // the kernel was measured with; wave_max on the key cast to int gave the same bits and 1.1 us more per call
  // (profiles/grid_common.md, first session).
  for (int sft = 32; sft > 0; sft >>= 1) {
    wkey = max(wkey, (unsigned)__shfl_xor((int)wkey, sft));
    wok += __shfl_xor(wok, sft);
  }
  if (lane == 0 && wkey) {
    atomicMax(&s_key, wkey);
    atomicAdd(&s_nok, wok);
  }
  __syncthreads();
  const unsigned win = s_key;
  if (win == 0u) {
    if (tid == 0) {
      Bst[0] = 0;
      Bst[1] = -1;
      Bst[2] = Bst[3] = Bst[4] = 0;
      Bst[5] = ax;
      Bst[6] = ay;
      Bst[7] = 0;
    }
  } else if (my_key == win) {
    Bst[0] = 1;
    Bst[1] = my_k;
    Bst[2] = my_m;
    Bst[3] = my_tlo;
    Bst[4] = my_w;
    Bst[5] = ax;
    Bst[6] = ay;
    Bst[7] = s_nok;
  }
}

bool shape_ok(int B, int G, int A, int M) {
  return batch_ok(B) && grid_ok(G) && A >= 1 && A <= MAX_A && M >= 0 && M <= MAX_M;
}

size_t ws_total(int B) { return align_up((size_t)B * NUM_IDS * MOM * sizeof(int), 256); }

}  // namespace
}  // namespace uoc

using namespace uoc;

extern "C" {

size_t uoc_grasp_workspace_bytes(int B, int G, int A, int M) {
  if (!shape_ok(B, G, A, M)) return 0;
  return ws_total(B);
}

int uoc_grasp(const int32_t *d_state, const int32_t *d_owner, int B, int G, const int32_t *h_dirs, int A, int M, int Wmax,
              int gap, int F, int Hp, int unknown_blocks, int32_t *d_cand, int32_t *d_best, void *d_ws, size_t ws_bytes,
              void *stream) {
  UOC_REQUIRE(d_state && d_owner && h_dirs && d_cand && d_best && d_ws, "uoc_grasp: null state / owner / dirs / cand / best / workspace");
  UOC_REQUIRE(batch_ok(B), "uoc_grasp: bad shape B=%d (B in 1..65535)", B);
  UOC_REQUIRE(grid_ok(G), "uoc_grasp: grid = %d is not a multiple of 8 in [8, %d]", G, MAX_G);
  UOC_REQUIRE(A >= 1 && A <= MAX_A, "uoc_grasp: %d directions outside [1, %d]", A, MAX_A);
  UOC_REQUIRE(M >= 0 && M <= MAX_M, "uoc_grasp: M = %d outside [0, %d]", M, MAX_M);
  UOC_REQUIRE(Wmax >= 1 && Wmax <= MAX_W, "uoc_grasp: Wmax = %d outside [1, %d]", Wmax, MAX_W);
  UOC_REQUIRE(gap >= 0 && gap <= MAX_GAP, "uoc_grasp: gap = %d outside [0, %d]", gap, MAX_GAP);
  UOC_REQUIRE(F >= 1 && F <= MAX_F, "uoc_grasp: F = %d outside [1, %d]", F, MAX_F);
  UOC_REQUIRE(Hp >= 0 && Hp <= MAX_HP, "uoc_grasp: Hp = %d outside [0, %d]", Hp, MAX_HP);
  UOC_REQUIRE(unknown_blocks == 0 || unknown_blocks == 1, "uoc_grasp: unknown_blocks = %d is neither 0 nor 1", unknown_blocks);
  Dirs d;
  for (int k = 0; k < MAX_A; ++k)
    for (int c = 0; c < 2; ++c) d.c[k][c] = k < A ? h_dirs[k * 2 + c] : 0;
  for (int k = 0; k < A; ++k)
    UOC_REQUIRE(d.c[k][0] >= -SCALE && d.c[k][0] <= SCALE && d.c[k][1] >= -SCALE && d.c[k][1] <= SCALE,
                "uoc_grasp: direction %d = (%d, %d) has a component outside [-%d, %d]", k, d.c[k][0], d.c[k][1], SCALE, SCALE);
  const size_t total = ws_total(B);
  UOC_REQUIRE(ws_bytes >= total, "uoc_grasp: workspace %zu < %zu bytes", ws_bytes, total);
  UOC_REQUIRE(aligned16(d_ws), "uoc_grasp: workspace not 16-byte aligned");
  Params p;
  p.G = G, p.A = A, p.M = M, p.Wmax = Wmax, p.gap = gap, p.F = F, p.Hp = Hp, p.unknown_blocks = unknown_blocks;
  p.R = 2 * Wmax;
  p.E = p.R + gap + F;
  p.T = 2 * p.E + 1;
  p.NLn = 2 * (M + Hp) + 1;
  p.KC = min(A, TABLE_CAP / (p.NLn * p.T));
  const size_t lds = (size_t)p.KC * p.NLn * p.T;
  const int cells = G * G;
  const double samples = (double)B * (NUM_IDS - 1) * A * p.NLn * p.T;
  hipStream_t st = (hipStream_t)stream;
  {
    ProfScope prof(KC_GRASP_MOMENTS, st, 0.0, (double)B * cells * 8.0);
    UOC_HIP_CHECK(hipMemsetAsync(d_ws, 0, total, st));
    hipLaunchKernelGGL(moments_kernel, dim3((cells + CHUNK - 1) / CHUNK, B), dim3(THREADS), 0, st, d_state, d_owner, G, (int *)d_ws);
  }
  {
    ProfScope prof(KC_GRASP_CANDIDATES, st, 0.0, samples * 8.0);
    hipLaunchKernelGGL(candidate_kernel, dim3(NUM_IDS, B), dim3(THREADS), lds, st, d_state, d_owner, (const int *)d_ws, d, p, d_cand,
                       d_best);
  }
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

}  // extern "C"
