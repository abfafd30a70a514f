// Scene memory: the table grid fused over time (include/uoc_hip.h, uoc_scene_step).  A per-stream memory
// of the state / owner grids of uoc_placement: observed cells overwrite it, cells not observed keep what was last seen
// there for at most max_age steps, contradictions are flagged and counted per id; then the clearance and the queries of
// uoc_placement on the fused grid.  Integers only.
//
// One memset (the per-id table, the info words and the query keys, accumulated in the workspace) and two launches, a
// third when there are queries:
//   update_kernel   grid (strips of STRIP columns, frames), STRIP * SEGS threads: placement.hip's column_kernel with the
//                   update in front.  Every block reads the frame's record, the stored one and the meta words (uniform
//                   across blocks: every block reaches the same status and restart decision) and does NOT write them:
//                   other blocks are still reading.  Per cell of the strip three words in (state, owner, memory) and six
//                   out (memory, state, owner, age, change and, after the scan, g); a thread loads its next 8 cells
//                   before it uses the first.  The per-id table is counted in LDS
//                   (128 x 8 words) and flushed once per block with integer atomics, `oldest` by atomicMax; the six info
//                   counters in registers, summed per wave by shuffles.
//   row_kernel      grid (rows, frames): grid.h's row pass and query keys.  Block (0, b) also copies the accumulated
//                   table and info words to the outputs, with the status and the step count, and stores the lattice
//                   record and the meta words: the launch that read them has finished.
//   answer_kernel   one block per frame: the keys back into (i, j, dist2, ok).
//
// Determinism: every count is a sum of ones, `oldest` a maximum, the query keys strict total orders; a cell's new word
// depends on that cell alone.  Nothing of stream b depends on the other streams of the batch.
#include "grid.h"

namespace uoc {
namespace {

constexpr int META = UOC_SCENE_META_WORD, MEM = UOC_SCENE_MEM_WORD;
constexpr int IDW = UOC_SCENE_ID_WORDS, INW = UOC_SCENE_INFO_WORDS;
constexpr int TABLE_WORDS = NUM_IDS * IDW;
constexpr int UNROLL = 8;  // cells per thread and turn of the update
enum { T_NOW = 0, T_KEPT, T_OLDEST, T_APPEARED, T_VANISHED, T_IN, T_OUT, T_FORGOTTEN };
enum { N_OBSERVED = 0, N_KEPT, N_FORGOTTEN, N_APPEARED, N_VANISHED, N_REOWNED, N_COUNTERS };

static_assert(META * 4 == NFR * 8 && MEM == META + 16, "the header: 16 int64, then 16 int32");
static_assert(2 + N_COUNTERS == INW, "info = status, steps and the six counters");
static_assert(NUM_IDS == 128, "the drop mask is four words");

__host__ __device__ inline size_t stream_words(int G) { return (size_t)MEM + (size_t)G * G; }

// Rule L: 0 no lattice, 1 step, 2 restart.  Uniform: every thread reads the same words.
__device__ __forceinline__ int lattice_status(const long long *__restrict__ rec, const int *__restrict__ hdr) {
  if (rec == nullptr) return 1;
  if (rec[FR_FOUND] != 1) return 0;
  if (hdr[META] > 0) {
    const long long *stored = reinterpret_cast<const long long *>(hdr);
    bool differs = false;
    for (int k = 0; k < NFR; ++k) differs |= rec[k] != stored[k];
    if (differs) return 2;
  }
  return 1;
}

// ---- 1. the update and the column pass ---------------------------------------------------------------------------------
__global__ __launch_bounds__(STRIP *SEGS) void update_kernel(const int *__restrict__ state_cur, const int *__restrict__ owner_cur,
                                                             const long long *__restrict__ frame, const int *__restrict__ drop,
                                                             int G, int max_age, int unknown_blocks, int *__restrict__ mem,
                                                             int *__restrict__ state, int *__restrict__ owner,
                                                             int *__restrict__ g_out, int *__restrict__ age,
                                                             int *__restrict__ change, int *__restrict__ acc_ids,
                                                             int *__restrict__ acc_info) {
  __shared__ unsigned short s[MAX_G][STRIP];  // bit 15: blocking; after the upward scan the low bits hold the distance up
  __shared__ int s_tab[TABLE_WORDS];
  __shared__ int s_cnt[N_COUNTERS];
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y, j0 = blockIdx.x * STRIP;
  int *hdr = mem + (size_t)b * stream_words(G);
  int *M = hdr + MEM;
  const int status = lattice_status(frame ? frame + (size_t)b * NFR : nullptr, hdr);
  unsigned dm[4] = {0u, 0u, 0u, 0u};
  if (drop)
    for (int k = 0; k < 4; ++k) dm[k] = (unsigned)drop[(size_t)b * 4 + k];
  const size_t off = (size_t)b * G * G;
  for (int t = tid; t < TABLE_WORDS; t += STRIP * SEGS) s_tab[t] = 0;
  if (tid < N_COUNTERS) s_cnt[tid] = 0;
  __syncthreads();
  int cnt[N_COUNTERS] = {};
  // UNROLL cells per thread and turn, every load of the turn issued before the first is used: a strip has few blocks, so
  // the pass is bound by the latency of its dependent loads, not by bytes.
  for (int base = tid; base < G * STRIP; base += UNROLL * STRIP * SEGS) {
    int sc[UNROLL], oc[UNROLL], mw[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int idx = base + u * STRIP * SEGS, i = idx / STRIP, j = j0 + idx % STRIP;
      sc[u] = oc[u] = mw[u] = 0;
      if (status != 0 && idx < G * STRIP && j < G) {
        const size_t c = (size_t)i * G + j;
        sc[u] = state_cur[off + c];
        oc[u] = owner_cur[off + c];
        if (status == 1) mw[u] = M[c];
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int idx = base + u * STRIP * SEGS, i = idx / STRIP, jj = idx % STRIP, j = j0 + jj;
      if (idx >= G * STRIP || j >= G) continue;
      const size_t c = (size_t)i * G + j;
      int st = 0, ow = 0, ag = -1, ch = UOC_SCENE_SAME;
      if (status != 0) {
        const int m = mw[u];
        const int ms = m & 0xFF, mo = (m >> 8) & (NUM_IDS - 1), ma = (m >> 16) & UOC_SCENE_MAX_AGE;  // a valid word's fields
        const int sn = (sc[u] == 1 || sc[u] == 2) ? sc[u] : 0;
        if (sn != 0) {  // observed
          st = sn;
          ow = (sn == 2 && oc[u] >= 1 && oc[u] < NUM_IDS) ? oc[u] : 0;
          ag = 0;
          ++cnt[N_OBSERVED];
          if (sn == 2) atomicAdd(&s_tab[ow * IDW + T_NOW], 1);
          if (ms == 1 && sn == 2) {
            ch = UOC_SCENE_APPEARED;
            ++cnt[N_APPEARED];
            atomicAdd(&s_tab[ow * IDW + T_APPEARED], 1);
          } else if (ms == 2 && sn == 1) {
            ch = UOC_SCENE_VANISHED;
            ++cnt[N_VANISHED];
            atomicAdd(&s_tab[mo * IDW + T_VANISHED], 1);
          } else if (ms == 2 && sn == 2 && mo != ow) {
            ch = UOC_SCENE_REOWNED;
            ++cnt[N_REOWNED];
            atomicAdd(&s_tab[ow * IDW + T_IN], 1);
            atomicAdd(&s_tab[mo * IDW + T_OUT], 1);
          }
        } else if (ms != 0) {
          const bool dropped = ms == 2 && ((dm[mo >> 5] >> (mo & 31)) & 1u);
          if (ma < max_age && !dropped) {  // kept
            st = ms;
            ow = mo;
            ag = ma + 1;
            ++cnt[N_KEPT];
            if (ms == 2) {
              atomicAdd(&s_tab[mo * IDW + T_KEPT], 1);
              atomicMax(&s_tab[mo * IDW + T_OLDEST], ag);
            }
          } else {  // forgotten
            ++cnt[N_FORGOTTEN];
            if (ms == 2) atomicAdd(&s_tab[mo * IDW + T_FORGOTTEN], 1);
          }
        }
        M[c] = ag < 0 ? 0 : (st | (ow << 8) | (ag << 16));
      }
      state[off + c] = st;
      owner[off + c] = ow;
      age[off + c] = ag;
      change[off + c] = ch;
      s[i][jj] = (status == 0 || st == 2 || (st == 0 && unknown_blocks)) ? 0x8000u : 0u;
    }
  }
#pragma unroll
  for (int k = 0; k < N_COUNTERS; ++k) {
    const int total = wave_sum(cnt[k]);
    if (lane == 0 && total) atomicAdd(&s_cnt[k], total);
  }
  __syncthreads();
  for (int t = tid; t < TABLE_WORDS; t += STRIP * SEGS) {
    const int v = s_tab[t];
    if (v == 0) continue;
    if ((t & (IDW - 1)) == T_OLDEST)
      atomicMax(&acc_ids[(size_t)b * TABLE_WORDS + t], v);
    else
      atomicAdd(&acc_ids[(size_t)b * TABLE_WORDS + t], v);
  }
  if (tid < N_COUNTERS && s_cnt[tid]) atomicAdd(&acc_info[(size_t)b * INW + 2 + tid], s_cnt[tid]);
  column_scan(s, G, j0, g_out + off);
}

// ---- 2. the row pass, the queries and the header -------------------------------------------------------------------------
__global__ __launch_bounds__(ROW_THREADS) void row_kernel(const int *__restrict__ state, const long long *__restrict__ frame, int G,
                                                          PlaceQueries qs, int Q, int *__restrict__ mem,
                                                          const int *__restrict__ acc_ids, const int *__restrict__ acc_info,
                                                          int *__restrict__ dist2, int *__restrict__ ids, int *__restrict__ info,
                                                          unsigned long long *__restrict__ keys) {
  if (blockIdx.x == 0) {  // uniform per block
    const int tid = threadIdx.x, b = blockIdx.y;
    int *hdr = mem + (size_t)b * stream_words(G);
    const long long *rec = frame ? frame + (size_t)b * NFR : nullptr;
    const int status = lattice_status(rec, hdr);
    const int steps = hdr[META], restarts = hdr[META + 1];
    long long word = 0;
    if (rec && tid < NFR) word = rec[tid];
    __syncthreads();  // every thread has read the header
    for (int t = tid; t < TABLE_WORDS; t += ROW_THREADS) ids[(size_t)b * TABLE_WORDS + t] = acc_ids[(size_t)b * TABLE_WORDS + t];
    if (tid < INW) info[(size_t)b * INW + tid] = tid == 0 ? status : tid == 1 ? steps + (status != 0) : acc_info[(size_t)b * INW + tid];
    if (status != 0) {
      if (rec && tid < NFR && (steps == 0 || status == 2)) reinterpret_cast<long long *>(hdr)[tid] = word;
      if (tid == 0) {
        hdr[META] = steps + 1;
        hdr[META + 1] = restarts + (status == 2);
      }
    }
  }
  row_pass_and_keys(state, G, qs, Q, dist2, keys);
}

__global__ __launch_bounds__(64) void answer_kernel(const unsigned long long *__restrict__ keys, int G, PlaceQueries qs, int Q,
                                                    int *__restrict__ answers) {
  answer_queries(keys, G, qs, Q, answers);
}

bool shape_ok(int B, int G) { return batch_ok(B) && grid_ok(G); }

struct Ws {
  int *ids;                  // [B][128][8]
  int *info;                 // [B][8]
  unsigned long long *keys;  // [B][PLACE_MAX_Q]
  size_t total;              // all of it zeroed per call
};
Ws carve(void *base, int B) {
  Ws w;
  Carver cv(base);
  w.ids = cv.take<int>((size_t)B * TABLE_WORDS);
  w.info = cv.take<int>((size_t)B * INW);
  w.keys = cv.take<unsigned long long>((size_t)B * PLACE_MAX_Q);
  w.total = cv.total();
  return w;
}

}  // namespace
}  // namespace uoc

using namespace uoc;

extern "C" {

size_t uoc_scene_state_bytes(int B, int G) {
  if (!shape_ok(B, G)) return 0;
  return (size_t)B * stream_words(G) * sizeof(int32_t);
}

size_t uoc_scene_workspace_bytes(int B, int G) {
  if (!shape_ok(B, G)) return 0;
  return carve(nullptr, B).total;
}

int uoc_scene_reset(void *d_state, int B, int G, int which, void *stream) {
  UOC_REQUIRE(d_state, "uoc_scene_reset: null state");
  UOC_REQUIRE(batch_ok(B), "uoc_scene_reset: bad shape B=%d (B in 1..65535)", B);
  UOC_REQUIRE(grid_ok(G), "uoc_scene_reset: grid = %d is not a multiple of 8 in [8, %d]", G, MAX_G);
  UOC_REQUIRE(which >= -1 && which < B, "uoc_scene_reset: which = %d outside [-1, %d]", which, B - 1);
  UOC_REQUIRE(aligned16(d_state), "uoc_scene_reset: state not 16-byte aligned");
  const size_t per = stream_words(G) * sizeof(int32_t);
  if (which < 0)
    UOC_HIP_CHECK(hipMemsetAsync(d_state, 0, per * B, (hipStream_t)stream));
  else
    UOC_HIP_CHECK(hipMemsetAsync((char *)d_state + per * which, 0, per, (hipStream_t)stream));
  return UOC_OK;
}

int uoc_scene_step(const int32_t *d_state_cur, const int32_t *d_owner_cur, const int64_t *d_frame, const int32_t *d_drop,
                   int B, int G, int max_age, int unknown_blocks, const int32_t *h_queries, int Q, void *d_mem,
                   int32_t *d_state, int32_t *d_owner, int32_t *d_dist2, int32_t *d_age, int32_t *d_change,
                   int32_t *d_ids, int32_t *d_info, int32_t *d_answers, void *d_ws, size_t ws_bytes, void *stream) {
  UOC_REQUIRE(d_state_cur && d_owner_cur && d_mem && d_state && d_owner && d_dist2 && d_age && d_change && d_ids && d_info && d_ws,
              "uoc_scene_step: null state_cur / owner_cur / memory / state / owner / dist2 / age / change / ids / info / workspace");
  UOC_REQUIRE(batch_ok(B), "uoc_scene_step: bad shape B=%d (B in 1..65535)", B);
  UOC_REQUIRE(grid_ok(G), "uoc_scene_step: grid = %d is not a multiple of 8 in [8, %d]", G, MAX_G);
  UOC_REQUIRE(max_age >= 0 && max_age <= UOC_SCENE_MAX_AGE, "uoc_scene_step: max_age = %d outside [0, %d]", max_age, UOC_SCENE_MAX_AGE);
  UOC_REQUIRE(unknown_blocks == 0 || unknown_blocks == 1, "uoc_scene_step: unknown_blocks = %d is neither 0 nor 1", unknown_blocks);
  PlaceQueries qs;
  if (const int rc = load_place_queries("uoc_scene_step", h_queries, d_answers, Q, qs)) return rc;
  const Ws w = carve(d_ws, B);
  UOC_REQUIRE(ws_bytes >= w.total, "uoc_scene_step: workspace %zu < %zu bytes", ws_bytes, w.total);
  UOC_REQUIRE(aligned16(d_ws), "uoc_scene_step: workspace not 16-byte aligned");
  UOC_REQUIRE(aligned16(d_mem), "uoc_scene_step: state not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long long *fr = (const long long *)d_frame;
  UOC_HIP_CHECK(hipMemsetAsync(d_ws, 0, w.total, st));
  hipLaunchKernelGGL(update_kernel, dim3((G + STRIP - 1) / STRIP, B), dim3(STRIP * SEGS), 0, st, d_state_cur, d_owner_cur, fr, d_drop, G,
                     max_age, unknown_blocks, (int *)d_mem, d_state, d_owner, d_dist2, d_age, d_change, w.ids, w.info);
  hipLaunchKernelGGL(row_kernel, dim3(G, B), dim3(ROW_THREADS), 0, st, d_state, fr, G, qs, Q, (int *)d_mem, w.ids, w.info, d_dist2,
                     d_ids, d_info, w.keys);
  if (Q > 0) hipLaunchKernelGGL(answer_kernel, dim3(B), dim3(64), 0, st, w.keys, G, qs, Q, d_answers);
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

}  // extern "C"
