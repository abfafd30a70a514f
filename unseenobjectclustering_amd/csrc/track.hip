// Object tracking across the frames of a stream (include/uoc_hip.h, uoc_track_*): every incoming label
// map becomes a tracked label map whose ids are track slots 1..127 that an object keeps while it is in view and gets
// back after a short occlusion.  B independent streams per call, no host round trip, integer arithmetic only.
//
// State per stream (caller-owned, uoc_track_state_bytes):
//   int32 [1024]     header: the slot table [128][5] = uid, age, hits, area, born (uoc_track), then at word META the
//                    number of uids handed out, the step counter and the sticky count of dropped objects
//   int32 [128][128] contingency table; all zero between steps (the matching kernel clears what it consumes)
//   int32 [H*W]      memory map: for every live track the pixels of its last sighting that nothing has covered since
// A zeroed state is a reset stream.
//
// One step is three launches on grids (block, stream):
//   cont_kernel   cont[mem][cur] over the pixels: a 128x128 table privatised in LDS per block, a wave adds each distinct
//                 pair once (wave_add_keys), blocks flush with integer atomics — integer adds commute, so the table
//                 does not depend on the order
//   match_kernel  one block of 1024 threads per stream: row / column sums, the candidate list (inter * 65536 >= q * union), greedy
//                 matching by exact IoU (cross-multiplied 64-bit integers; ties: larger inter, lower track, lower id) run by
//                 wave 0 alone so that a round costs no block barrier, then ageing, births (rank among the unmatched
//                 ids -> rank among the free slots, by ballot prefix sums), the lut and the keep flags of the memory map
//   apply_kernel  out = lut[cur]; mem' = out where out != 0, else mem where its track is kept, else 0
//
// The pixel kernels read and write int4 when H*W is a multiple of 4 and the maps are 16-byte aligned, else one int.
#include "labelmap.h"

#include <limits.h>

namespace uoc {
namespace {

constexpr int HDR_WORDS = 1024;             // header words per stream
constexpr int META = NUM_IDS * 5;           // header word of {uids handed out, step, dropped}
constexpr int CONT_WORDS = NUM_IDS * NUM_IDS;
constexpr int CONT_THREADS = 1024;
constexpr int PIX_PER_BLOCK = CONT_THREADS * 8;   // pixels per contingency block until MAX_BLOCKS is reached
constexpr int MAX_BLOCKS = 64;              // pixel-kernel blocks per stream (grid-stride beyond)
constexpr int MATCH_THREADS = 1024;
constexpr int PLAN_WORDS = 2 * NUM_IDS;     // workspace per stream: lut[128], keep[128]

static_assert(sizeof(uoc_track) == 5 * sizeof(int32_t), "uoc_track is five int32");

inline size_t state_stride(long long n) {
  return align_up((size_t)(HDR_WORDS + CONT_WORDS) * 4 + (size_t)n * 4, 256);
}
__device__ __forceinline__ int *state_hdr(void *state, size_t stride, int b) { return (int *)((char *)state + stride * b); }

// Table index of a pixel.  The memory map only ever holds 0..127; the mask keeps a state that was never reset in bounds.
__device__ __forceinline__ int pair_key(int m, int l) { return (m & (NUM_IDS - 1)) * NUM_IDS + obj_id(l); }

// ---- 1. contingency ------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(CONT_THREADS) void cont_kernel(const int *__restrict__ labels, void *__restrict__ state,
                                                            size_t stride, int n) {
  __shared__ int s_cont[CONT_WORDS];
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y;
  for (int i = tid; i < CONT_WORDS / 4; i += CONT_THREADS) reinterpret_cast<int4 *>(s_cont)[i] = make_int4(0, 0, 0, 0);
  __syncthreads();
  int *hdr = state_hdr(state, stride, b);
  int *cont = hdr + HDR_WORDS;
  const int *M = cont + CONT_WORDS;
  const int *L = labels + (size_t)b * n;
  const long long nv = n / V;   // V == 4 only when n % 4 == 0
  const long long step = (long long)gridDim.x * CONT_THREADS;
  for (long long base = (long long)blockIdx.x * CONT_THREADS + (tid - lane); base < nv; base += step) {  // wave-uniform
    const long long i = base + lane;
    const bool act = i < nv;
    if (V == 4) {
      int4 l = make_int4(0, 0, 0, 0), m = make_int4(0, 0, 0, 0);
      if (act) {
        l = reinterpret_cast<const int4 *>(L)[i];
        m = reinterpret_cast<const int4 *>(M)[i];
      }
      const int k0 = act ? pair_key(m.x, l.x) : -1, k1 = act ? pair_key(m.y, l.y) : -1;
      const int k2 = act ? pair_key(m.z, l.z) : -1, k3 = act ? pair_key(m.w, l.w) : -1;
      if (__all(k0 == k1 && k1 == k2 && k2 == k3)) {   // the usual case: every lane's four pixels are one pair
        wave_add_keys(s_cont, k0, 4, lane);
      } else {
        wave_add_keys(s_cont, k0, 1, lane);
        wave_add_keys(s_cont, k1, 1, lane);
        wave_add_keys(s_cont, k2, 1, lane);
        wave_add_keys(s_cont, k3, 1, lane);
      }
    } else {
      const int k = act ? pair_key(M[i], L[i]) : -1;
      wave_add_keys(s_cont, k, 1, lane);
    }
  }
  __syncthreads();
  for (int i = tid; i < CONT_WORDS / 4; i += CONT_THREADS) {
    const int4 v = reinterpret_cast<const int4 *>(s_cont)[i];
    if (v.x) atomicAdd(&cont[4 * i + 0], v.x);
    if (v.y) atomicAdd(&cont[4 * i + 1], v.y);
    if (v.z) atomicAdd(&cont[4 * i + 2], v.z);
    if (v.w) atomicAdd(&cont[4 * i + 3], v.w);
  }
}

// ---- 2. matching, ageing, births ------------------------------------------------------------------------------------
struct Cand {
  int inter, uni, key;   // key = track * 128 + id; the empty candidate is {0, 1, INT_MAX}
};
// a before b: larger IoU (exact), then larger intersection, then lower track, then lower id
__device__ __forceinline__ bool better(const Cand &a, const Cand &b) {
  const unsigned long long l = (unsigned long long)a.inter * (unsigned)b.uni, r = (unsigned long long)b.inter * (unsigned)a.uni;
  if (l != r) return l > r;
  if (a.inter != b.inter) return a.inter > b.inter;
  return a.key < b.key;
}
// The best candidate of the wave, in every lane: a DPP tree per 16-lane row, then the four rows.  All 64 lanes active.
template <int CTRL>
__device__ __forceinline__ Cand dpp_best(const Cand &v) {
  const Cand o{dpp_i<CTRL>(v.inter), dpp_i<CTRL>(v.uni), dpp_i<CTRL>(v.key)};
  return better(o, v) ? o : v;
}
__device__ __forceinline__ Cand lane_of(const Cand &v, int lane) {
  return Cand{__builtin_amdgcn_readlane(v.inter, lane), __builtin_amdgcn_readlane(v.uni, lane),
              __builtin_amdgcn_readlane(v.key, lane)};
}
__device__ __forceinline__ Cand wave_best(Cand v) {
  v = dpp_best<0xB1>(v);
  v = dpp_best<0x4E>(v);
  v = dpp_best<0x141>(v);
  v = dpp_best<0x140>(v);
  Cand r = lane_of(v, 0);
  const Cand r1 = lane_of(v, 16), r2 = lane_of(v, 32), r3 = lane_of(v, 48);
  if (better(r1, r)) r = r1;
  if (better(r2, r)) r = r2;
  if (better(r3, r)) r = r3;
  return r;
}

__global__ __launch_bounds__(MATCH_THREADS) void match_kernel(void *__restrict__ state, size_t stride, int q, int max_age,
                                                              int *__restrict__ plan, int *__restrict__ lut_out,
                                                              uoc_track *__restrict__ tracks_out) {
  extern __shared__ int s_dyn[];
  int *s_cont = s_dyn;                                              // [128][128]
  unsigned short *s_list = (unsigned short *)(s_dyn + CONT_WORDS);  // candidate keys, at most 127 * 127
  __shared__ int area_mem[NUM_IDS], area_cur[NUM_IDS], s_uid[NUM_IDS], match_t[NUM_IDS], match_c[NUM_IDS];
  __shared__ int s_lut[NUM_IDS], s_keep[NUM_IDS];
  __shared__ int slot_of_rank[NUM_IDS], born_uid[NUM_IDS], born_area[NUM_IDS];
  __shared__ int s_nlist, s_cnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  int *hdr = state_hdr(state, stride, b);
  int *cont = hdr + HDR_WORDS;

  // the slot this thread owns (tid < 128)
  int uid = 0, age = 0, hits = 0, area = 0, born = 0;
  if (tid < NUM_IDS) {
    uid = hdr[tid * 5 + 0];
    age = hdr[tid * 5 + 1];
    hits = hdr[tid * 5 + 2];
    area = hdr[tid * 5 + 3];
    born = hdr[tid * 5 + 4];
    if (tid == 0) uid = 0;   // slot 0 is never a track
    s_uid[tid] = uid;
    match_t[tid] = match_c[tid] = s_lut[tid] = s_keep[tid] = born_uid[tid] = born_area[tid] = 0;
  }
  if (tid == 0) s_nlist = 0;
  const int issued = hdr[META + 0], step = hdr[META + 1], dropped = hdr[META + 2];
  {   // stage the table and leave it zero for the next step; all of a thread's loads are in flight together
    constexpr int PER = CONT_WORDS / 4 / MATCH_THREADS;
    int4 v[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) v[k] = reinterpret_cast<const int4 *>(cont)[tid + k * MATCH_THREADS];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      reinterpret_cast<int4 *>(s_cont)[tid + k * MATCH_THREADS] = v[k];
      if (v[k].x | v[k].y | v[k].z | v[k].w) reinterpret_cast<int4 *>(cont)[tid + k * MATCH_THREADS] = make_int4(0, 0, 0, 0);
    }
  }
  __syncthreads();

  if (tid < NUM_IDS) {   // row sums; the column index is rotated by the row so that the lanes fall on different banks
    int s = 0;
    for (int j = 0; j < NUM_IDS; ++j) s += s_cont[tid * NUM_IDS + ((j + tid) & (NUM_IDS - 1))];
    area_mem[tid] = s;
  } else if (tid < 2 * NUM_IDS) {   // column sums
    const int c = tid - NUM_IDS;
    int s = 0;
    for (int t = 0; t < NUM_IDS; ++t) s += s_cont[t * NUM_IDS + c];
    area_cur[c] = s;
  }
  __syncthreads();

  for (int i = tid; i < CONT_WORDS; i += MATCH_THREADS) {   // candidates
    const int t = i >> 7, c = i & (NUM_IDS - 1), inter = s_cont[i];
    if (t >= 1 && c >= 1 && inter > 0 && s_uid[t] != 0) {
      const long long uni = (long long)area_mem[t] + area_cur[c] - inter;
      if ((long long)inter * 65536 >= (long long)q * uni) s_list[atomicAdd(&s_nlist, 1)] = (unsigned short)i;
    }
  }
  __syncthreads();

  if (wave == 0) {   // greedy rounds; every lane ends a round with the same winner, so the matched sets stay in registers
    const int nlist = s_nlist;
    unsigned long long mt0 = 0ull, mt1 = 0ull, mc0 = 0ull, mc1 = 0ull;
    for (;;) {
      Cand best{0, 1, INT_MAX};
      for (int k = lane; k < nlist; k += 64) {
        const int key = s_list[k], t = key >> 7, c = key & (NUM_IDS - 1);
        if ((((t & 64 ? mt1 : mt0) >> (t & 63)) | ((c & 64 ? mc1 : mc0) >> (c & 63))) & 1ull) continue;
        const int inter = s_cont[key];
        const Cand cand{inter, area_mem[t] + (area_cur[c] - inter), key};
        if (better(cand, best)) best = cand;
      }
      best = wave_best(best);
      if (best.inter == 0) break;   // the same in every lane
      const int t = best.key >> 7, c = best.key & (NUM_IDS - 1);
      (t & 64 ? mt1 : mt0) |= 1ull << (t & 63);
      (c & 64 ? mc1 : mc0) |= 1ull << (c & 63);
      if (lane == 0) {
        match_t[t] = c;
        match_c[c] = t;
      }
    }
  }
  __syncthreads();

  if (tid >= 1 && tid < NUM_IDS && uid != 0) {   // ageing
    const int c = match_t[tid];
    if (c) {
      age = 0;
      hits += 1;
      area = area_cur[c];
      s_lut[c] = tid;
    } else {
      age += 1;
      if (age > max_age)
        uid = age = hits = area = born = 0;   // retired: the slot is free again
      else
        s_keep[tid] = 1;                      // occluded: its footprint stays in the memory map
    }
    s_uid[tid] = uid;
  }
  __syncthreads();

  // births: the unmatched present ids in ascending order take the free slots in ascending order
  const bool is_new = tid >= 1 && tid < NUM_IDS && area_cur[tid] > 0 && match_c[tid] == 0;
  const bool is_free = tid >= 1 && tid < NUM_IDS && s_uid[tid] == 0;
  const unsigned long long bal_new = __ballot(is_new), bal_free = __ballot(is_free);
  if (wave < 2 && lane == 0) {
    s_cnt[wave] = (int)__popcll(bal_new);
    s_cnt[2 + wave] = (int)__popcll(bal_free);
  }
  __syncthreads();
  const int n_new = s_cnt[0] + s_cnt[1], n_free = s_cnt[2] + s_cnt[3];
  const int rank_new = lane_rank(bal_new) + (wave == 1 ? s_cnt[0] : 0);
  const int rank_free = lane_rank(bal_free) + (wave == 1 ? s_cnt[2] : 0);
  if (is_free) slot_of_rank[rank_free] = tid;
  __syncthreads();
  if (is_new && rank_new < n_free) {
    const int s = slot_of_rank[rank_new];
    s_lut[tid] = s;
    born_uid[s] = issued + 1 + rank_new;
    born_area[s] = area_cur[tid];
  }
  __syncthreads();

  if (tid < NUM_IDS) {
    if (born_uid[tid]) {
      uid = born_uid[tid];
      age = 0;
      hits = 1;
      area = born_area[tid];
      born = step;
    }
    hdr[tid * 5 + 0] = uid;
    hdr[tid * 5 + 1] = age;
    hdr[tid * 5 + 2] = hits;
    hdr[tid * 5 + 3] = area;
    hdr[tid * 5 + 4] = born;
    if (tracks_out) tracks_out[(size_t)b * NUM_IDS + tid] = uoc_track{uid, age, hits, area, born};
    plan[(size_t)b * PLAN_WORDS + tid] = s_lut[tid];
    plan[(size_t)b * PLAN_WORDS + NUM_IDS + tid] = s_keep[tid];
    if (lut_out) lut_out[(size_t)b * NUM_IDS + tid] = s_lut[tid];
  }
  if (tid == 0) {
    const int births = n_new < n_free ? n_new : n_free;
    hdr[META + 0] = issued + births;
    hdr[META + 1] = step + 1;
    hdr[META + 2] = dropped + (n_new - births);
  }
}

// ---- 3. tracked map and memory map -----------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void apply_kernel(const int *__restrict__ labels, void *__restrict__ state, size_t stride,
                                                    int n, const int *__restrict__ plan, int *__restrict__ out) {
  __shared__ int s_lut[NUM_IDS], s_keep[NUM_IDS];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (tid < NUM_IDS) {
    s_lut[tid] = plan[(size_t)b * PLAN_WORDS + tid];
    s_keep[tid] = plan[(size_t)b * PLAN_WORDS + NUM_IDS + tid];
  }
  __syncthreads();
  int *M = state_hdr(state, stride, b) + HDR_WORDS + CONT_WORDS;
  const int *L = labels + (size_t)b * n;
  int *O = out + (size_t)b * n;
  const long long nv = n / V, step = (long long)gridDim.x * 256;
  auto one = [&](int l, int m, int &o, int &mm) {
    o = s_lut[obj_id(l)];
    mm = o ? o : (s_keep[m & (NUM_IDS - 1)] ? m : 0);
  };
  for (long long i = (long long)blockIdx.x * 256 + tid; i < nv; i += step) {
    if (V == 4) {
      const int4 l = reinterpret_cast<const int4 *>(L)[i], m = reinterpret_cast<const int4 *>(M)[i];
      int4 o, mm;
      one(l.x, m.x, o.x, mm.x);
      one(l.y, m.y, o.y, mm.y);
      one(l.z, m.z, o.z, mm.z);
      one(l.w, m.w, o.w, mm.w);
      reinterpret_cast<int4 *>(O)[i] = o;
      reinterpret_cast<int4 *>(M)[i] = mm;
    } else {
      int o, mm;
      one(L[i], M[i], o, mm);
      O[i] = o;
      M[i] = mm;
    }
  }
}

int check_shape(const char *who, int B, int H, int W) {
  UOC_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
  UOC_REQUIRE((long long)H * W <= INT_MAX, "%s: H*W = %lld does not fit 31 bits", who, (long long)H * W);
  return UOC_OK;
}

}  // namespace
}  // namespace uoc

using namespace uoc;

extern "C" {

size_t uoc_track_state_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || (long long)H * W > INT_MAX) return 0;
  return state_stride((long long)H * W) * (size_t)B;
}

size_t uoc_track_workspace_bytes(int B) {
  if (B <= 0) return 0;
  return (size_t)B * PLAN_WORDS * sizeof(int32_t);
}

int uoc_track_reset(void *d_state, int B, int H, int W, int which, void *stream) {
  UOC_REQUIRE(d_state, "uoc_track_reset: null state");
  if (int rc = check_shape("uoc_track_reset", B, H, W)) return rc;
  UOC_REQUIRE(which >= -1 && which < B, "uoc_track_reset: stream %d outside [-1, %d)", which, B);
  const size_t stride = state_stride((long long)H * W);
  if (which < 0)
    UOC_HIP_CHECK(hipMemsetAsync(d_state, 0, stride * (size_t)B, (hipStream_t)stream));
  else
    UOC_HIP_CHECK(hipMemsetAsync((char *)d_state + stride * (size_t)which, 0, stride, (hipStream_t)stream));
  return UOC_OK;
}

int uoc_track_step(const int32_t *d_labels, int B, int H, int W, int q, int max_age, void *d_state, int32_t *d_out,
                   int32_t *d_lut, uoc_track *d_tracks, void *d_ws, size_t ws_bytes, void *stream) {
  UOC_REQUIRE(d_labels && d_state && d_out && d_ws, "uoc_track_step: null labels / state / out / workspace");
  if (int rc = check_shape("uoc_track_step", B, H, W)) return rc;
  UOC_REQUIRE(q >= 1 && q <= 65536, "uoc_track_step: q = %d outside [1, 65536] (q = round(min_iou * 65536))", q);
  UOC_REQUIRE(max_age >= 0, "uoc_track_step: max_age = %d is negative", max_age);
  UOC_REQUIRE(ws_bytes >= uoc_track_workspace_bytes(B), "uoc_track_step: workspace %zu < %zu bytes", ws_bytes,
              uoc_track_workspace_bytes(B));
  UOC_REQUIRE((((uintptr_t)d_state | (uintptr_t)d_ws) & 15) == 0, "uoc_track_step: state / workspace not 16-byte aligned");
  const int n = H * W;
  const size_t stride = state_stride(n);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)CONT_WORDS * 4 + (size_t)CONT_WORDS * 2;
  static DeviceOnce attr_set;
  if (int rc = opt_in_dynamic_lds(reinterpret_cast<const void *>(&match_kernel), lds, attr_set)) return rc;
  const bool vec = n % 4 == 0 && (((uintptr_t)d_labels | (uintptr_t)d_out) & 15) == 0;
  int blocks = (n + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK;
  if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
  int *plan = (int *)d_ws;
  if (vec)
    hipLaunchKernelGGL(cont_kernel<4>, dim3(blocks, B), dim3(CONT_THREADS), 0, st, d_labels, d_state, stride, n);
  else
    hipLaunchKernelGGL(cont_kernel<1>, dim3(blocks, B), dim3(CONT_THREADS), 0, st, d_labels, d_state, stride, n);
  hipLaunchKernelGGL(match_kernel, dim3(B), dim3(MATCH_THREADS), lds, st, d_state, stride, q, max_age, plan, d_lut, d_tracks);
  const int ablocks = blocks * 4;   // 256-thread blocks over the same pixels
  if (vec)
    hipLaunchKernelGGL(apply_kernel<4>, dim3(ablocks, B), dim3(256), 0, st, d_labels, d_state, stride, n, plan, d_out);
  else
    hipLaunchKernelGGL(apply_kernel<1>, dim3(ablocks, B), dim3(256), 0, st, d_labels, d_state, stride, n, plan, d_out);
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

}  // extern "C"
