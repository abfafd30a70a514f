// Re-identification (include/uoc_hip.h, uoc_signature / uoc_sig_similarity / uoc_ident_*): an appearance
// signature per object of a label map, the similarity of two signatures, and per stream a table of identities that binds
// a new track to the lost identity it looks like.  Integer arithmetic only (the one rintf is labelmap.h's depth_mm
// rule), so every result is defined exactly and does not depend on launch order or batch.
//
// Signatures are two launches on grids (block, stream) and (id, stream):
//   sig_kernel     per block a table [128][91] of vote counters and the header counters in LDS; a pixel votes with LDS
//                  atomics, a wave adds pixels / valid / area once per distinct id (for_each_wave_key); blocks flush
//                  their non-zero cells with integer atomics into the accumulator in the workspace
//   sig_finish     normalises an id's row into d_sig and puts the accumulator's row back to zero: the accumulator is
//                  all zero between calls and no call needs a memset
// The pixel kernel reads int4 labels, three words of BGR and a float4 of z per lane when H*W is a multiple of 4 and the
// pointers allow it, else one pixel per lane.
//
// One identity step is two launches:
//   ident_kernel   one block of 1024 threads per stream: forgetting, binding by uid, the candidate list (pair_similarity
//                  and the size gate) in LDS, greedy matching run by wave 0 alone on one packed 64-bit key per candidate
//                  (wave_max64 over a strict total order), new entries and evictions by rank, then the table, the
//                  counters and the stored signatures
//   relabel_kernel out = lut[tracked]
#include "labelmap.h"

#include <limits.h>

namespace uoc {
namespace {

constexpr int SIG = UOC_SIG_WORDS;          // words per signature
constexpr int HIST0 = UOC_SIG_HIST;         // first histogram word
constexpr int CHROMA = 81;                  // 9 x 9 chromaticity bins, then the dark bin, then 9 intensity bins
constexpr int NHIST = CHROMA + 1 + 9;
constexpr int SIG_THREADS = 1024;
constexpr int PIX_PER_BLOCK = SIG_THREADS * 8;
constexpr int MAX_BLOCKS = 64;              // pixel-kernel blocks per stream (grid-stride beyond)

constexpr int HDR_WORDS = UOC_IDENT_HEADER_WORDS;   // state: the table [128][5], the counters at META, then the signatures
constexpr int META = UOC_IDENT_META_WORD;
constexpr int ENT = UOC_IDENT_WORDS;                // pid, uid, seen, hits, pixels
constexpr int STATE_WORDS = HDR_WORDS + NUM_IDS * SIG;
constexpr int IDENT_THREADS = 1024;
constexpr int MAX_CAND = (NUM_IDS - 1) * (NUM_IDS - 1);

static_assert(HIST0 + NHIST == UOC_SIG_DARK + 10 && UOC_SIG_DARK == HIST0 + CHROMA && HIST0 + NHIST <= SIG, "signature layout");
static_assert(META + 3 <= HDR_WORDS && NUM_IDS * ENT <= META && (STATE_WORDS * 4) % 256 == 0, "identity state layout");
static_assert(sizeof(uoc_track) == 5 * sizeof(int32_t), "uoc_track is five int32");

__device__ __forceinline__ unsigned area_of(int zmm) { return zmm >= 0 ? ((unsigned)zmm * (unsigned)zmm) >> 10 : 0u; }

// ---- 1. signatures --------------------------------------------------------------------------------------------------
// The votes of one pixel into its id's row h[91]: 64 to the chroma / dark part, 64 to the intensity part.
__device__ __forceinline__ void vote(unsigned *__restrict__ h, unsigned b, unsigned g, unsigned r) {
  const unsigned s = b + g + r;
  if (s >= 48u) {
    const unsigned u = (64u * b) / s, v = (64u * g) / s;   // u + v <= 64
    const unsigned ul = u >> 3, uf = u & 7u, vl = v >> 3, vf = v & 7u;
    unsigned *c = h + ul * 9u + vl;
    atomicAdd(c, (8u - uf) * (8u - vf));
    if (vf) atomicAdd(c + 1, (8u - uf) * vf);
    if (uf) atomicAdd(c + 9, uf * (8u - vf));
    if (uf && vf) atomicAdd(c + 10, uf * vf);                // zero weights are skipped: ul == 8 has uf == 0
  } else {
    atomicAdd(h + CHROMA, 64u);
  }
  const unsigned y = s / 3u, yl = y >> 5, yf = (y & 31u) >> 2;
  atomicAdd(h + CHROMA + 1 + yl, 8u * (8u - yf));
  if (yf) atomicAdd(h + CHROMA + 2 + yl, 8u * yf);
}

// pixels, valid and area of the wave's lanes, once per distinct id.  cnt pixels per lane, of which nvalid have a depth;
// area is the lane's sum (at most 4 * 65000^2 >> 10, so the wave's sum stays below 2^31).
__device__ __forceinline__ void wave_header(unsigned *__restrict__ s_pix, unsigned *__restrict__ s_valid,
                                            unsigned long long *__restrict__ s_area, int key, int cnt, int nvalid, int area,
                                            int lane) {
  for_each_wave_key(key, [&](int c, unsigned long long m, int first) {
    const bool mine = key == c;
    const int pv = wave_sum(mine ? nvalid : 0), ar = wave_sum(mine ? area : 0);
    if (lane == first) {
      atomicAdd(&s_pix[c], (unsigned)(cnt * (int)__popcll(m)));
      if (pv) atomicAdd(&s_valid[c], (unsigned)pv);
      if (ar) atomicAdd(&s_area[c], (unsigned long long)ar);
    }
  });
}

template <int V>
__global__ __launch_bounds__(SIG_THREADS) void sig_kernel(const int *__restrict__ labels, const uint8_t *__restrict__ image,
                                                          const float *__restrict__ xyz, unsigned *__restrict__ acc, int n) {
  __shared__ unsigned s_hist[NUM_IDS * NHIST];
  __shared__ unsigned s_pix[NUM_IDS], s_valid[NUM_IDS];
  __shared__ unsigned long long s_area[NUM_IDS];
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y;
  for (int i = tid; i < NUM_IDS * NHIST; i += SIG_THREADS) s_hist[i] = 0u;
  if (tid < NUM_IDS) {
    s_pix[tid] = s_valid[tid] = 0u;
    s_area[tid] = 0ull;
  }
  __syncthreads();
  const int *L = labels + (size_t)b * n;
  const uint8_t *I = image + (size_t)b * n * 3;
  const float *Z = xyz ? xyz + ((size_t)b * 3 + 2) * n : nullptr;
  const long long nv = n / V;   // V == 4 only when n % 4 == 0
  const long long step = (long long)gridDim.x * SIG_THREADS;
  for (long long base = (long long)blockIdx.x * SIG_THREADS + (tid - lane); base < nv; base += step) {  // wave-uniform
    const long long i = base + lane;
    const bool act = i < nv;
    if (V == 4) {
      int4 l = make_int4(0, 0, 0, 0);
      unsigned c0 = 0u, c1 = 0u, c2 = 0u;
      float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      if (act) {
        l = reinterpret_cast<const int4 *>(L)[i];
        const unsigned *w = reinterpret_cast<const unsigned *>(I) + 3 * i;   // four BGR pixels are three words
        c0 = w[0];
        c1 = w[1];
        c2 = w[2];
        if (Z) z = reinterpret_cast<const float4 *>(Z)[i];
      }
      const int k0 = act ? obj_key(l.x) : -1, k1 = act ? obj_key(l.y) : -1;
      const int k2 = act ? obj_key(l.z) : -1, k3 = act ? obj_key(l.w) : -1;
      if (k0 >= 0) vote(s_hist + k0 * NHIST, c0 & 255u, (c0 >> 8) & 255u, (c0 >> 16) & 255u);
      if (k1 >= 0) vote(s_hist + k1 * NHIST, c0 >> 24, c1 & 255u, (c1 >> 8) & 255u);
      if (k2 >= 0) vote(s_hist + k2 * NHIST, (c1 >> 16) & 255u, c1 >> 24, c2 & 255u);
      if (k3 >= 0) vote(s_hist + k3 * NHIST, (c2 >> 8) & 255u, (c2 >> 16) & 255u, c2 >> 24);
      const int z0 = Z ? depth_mm(z.x) : -1, z1 = Z ? depth_mm(z.y) : -1, z2 = Z ? depth_mm(z.z) : -1, z3 = Z ? depth_mm(z.w) : -1;
      if (__all(k0 == k1 && k1 == k2 && k2 == k3)) {   // the usual case: every lane's four pixels are one id
        wave_header(s_pix, s_valid, s_area, k0, 4, (z0 >= 0) + (z1 >= 0) + (z2 >= 0) + (z3 >= 0),
                    (int)(area_of(z0) + area_of(z1) + area_of(z2) + area_of(z3)), lane);
      } else {
        wave_header(s_pix, s_valid, s_area, k0, 1, z0 >= 0, (int)area_of(z0), lane);
        wave_header(s_pix, s_valid, s_area, k1, 1, z1 >= 0, (int)area_of(z1), lane);
        wave_header(s_pix, s_valid, s_area, k2, 1, z2 >= 0, (int)area_of(z2), lane);
        wave_header(s_pix, s_valid, s_area, k3, 1, z3 >= 0, (int)area_of(z3), lane);
      }
    } else {
      const int k = act ? obj_key(L[i]) : -1;
      if (k >= 0) vote(s_hist + k * NHIST, I[3 * i], I[3 * i + 1], I[3 * i + 2]);
      const int zq = (act && Z) ? depth_mm(Z[i]) : -1;
      wave_header(s_pix, s_valid, s_area, k, 1, zq >= 0, (int)area_of(zq), lane);
    }
  }
  __syncthreads();
  unsigned *A = acc + (size_t)b * NUM_IDS * SIG;
  for (int i = tid; i < NUM_IDS * NHIST; i += SIG_THREADS) {
    const unsigned v = s_hist[i];
    if (v) atomicAdd(&A[(i / NHIST) * SIG + HIST0 + i % NHIST], v);
  }
  if (tid < NUM_IDS) {
    if (s_pix[tid]) atomicAdd(&A[tid * SIG + UOC_SIG_PIXELS], s_pix[tid]);
    if (s_valid[tid]) atomicAdd(&A[tid * SIG + UOC_SIG_VALID], s_valid[tid]);
    if (s_area[tid]) atomicAdd(reinterpret_cast<unsigned long long *>(&A[tid * SIG + UOC_SIG_AREA]), s_area[tid]);
  }
}

// One block per (id, stream), one thread per word: reads the row, then writes the signature and zeroes the row.
__global__ __launch_bounds__(NUM_IDS) void sig_finish(unsigned *__restrict__ acc, int *__restrict__ sig) {
  const int k = threadIdx.x;
  const size_t row = ((size_t)blockIdx.y * NUM_IDS + blockIdx.x) * SIG;
  const unsigned n = acc[row + UOC_SIG_PIXELS];
  const unsigned h = k < SIG ? acc[row + k] : 0u;
  __syncthreads();   // every thread has read n before the thread of word 0 clears it
  if (k >= SIG) return;
  unsigned out = h;
  if (k >= HIST0 && k < HIST0 + NHIST)
    out = n ? (unsigned)(((unsigned long long)h * (k <= UOC_SIG_DARK ? 768u : 256u)) / n) : 0u;
  sig[row + k] = (int)out;
  if (h) acc[row + k] = 0u;
}

// ---- 2. similarity ----------------------------------------------------------------------------------------------------
// The pair function of uoc_sig_similarity and of the identity step: the histogram intersection of two signatures, 0 when
// either has no pixels.  Rows are 16-byte aligned; words 8..99 are 23 int4, of which word 99 is no histogram word.
__device__ __forceinline__ int pair_similarity(const int *__restrict__ qa, const int *__restrict__ qb) {
  if (qa[UOC_SIG_PIXELS] <= 0 || qb[UOC_SIG_PIXELS] <= 0) return 0;
  const int4 *a = reinterpret_cast<const int4 *>(qa + HIST0), *b = reinterpret_cast<const int4 *>(qb + HIST0);
  int s = 0;
#pragma unroll
  for (int k = 0; k < 23; ++k) {
    const int4 x = a[k], y = b[k];
    s += min(x.x, y.x) + min(x.y, y.y) + min(x.z, y.z);
    if (k < 22) s += min(x.w, y.w);
  }
  return s;
}

__global__ __launch_bounds__(NUM_IDS) void sim_kernel(const int *__restrict__ sa, const int *__restrict__ sb, int *__restrict__ sim) {
  const size_t t = (size_t)blockIdx.y * NUM_IDS;
  sim[(t + blockIdx.x) * NUM_IDS + threadIdx.x] = pair_similarity(sa + (t + blockIdx.x) * SIG, sb + (t + threadIdx.x) * SIG);
}

// ---- 3. identities ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long area64(const int *__restrict__ q) {
  return (unsigned long long)(unsigned)q[UOC_SIG_AREA] | ((unsigned long long)(unsigned)q[UOC_SIG_AREA + 1] << 32);
}

__global__ __launch_bounds__(IDENT_THREADS) void ident_kernel(const uoc_track *__restrict__ tracks, const int *__restrict__ sig,
                                                              int *__restrict__ state, int q, int r, int max_lost,
                                                              int *__restrict__ plan, int *__restrict__ lut_out,
                                                              int *__restrict__ ident_out) {
  extern __shared__ unsigned s_list[];   // candidates: sim << 14 | slot << 7 | entry, at most 127 * 127
  __shared__ int s_tuid[NUM_IDS], s_pid[NUM_IDS], s_euid[NUM_IDS], s_seen[NUM_IDS], s_ent_of[NUM_IDS], s_slot_of[NUM_IDS];
  __shared__ int s_new[NUM_IDS], s_lost[NUM_IDS], s_free[NUM_IDS], s_free_at[NUM_IDS], s_lost_at[NUM_IDS], s_newpid[NUM_IDS];
  __shared__ unsigned long long s_anew[NUM_IDS], s_aold[NUM_IDS];
  __shared__ int s_nlist;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  int *hdr = state + (size_t)b * STATE_WORDS;
  int *esig = hdr + HDR_WORDS;
  const int *S = sig + (size_t)b * NUM_IDS * SIG;
  const uoc_track *T = tracks + (size_t)b * NUM_IDS;
  const int pids = hdr[META + 0], step = hdr[META + 1] + 1, evicted = hdr[META + 2];

  // 1. the entry this thread owns (tid < 128), forgotten when it was lost for too long; 2. the slot it owns
  int pid = 0, uid = 0, seen = 0, hits = 0, pixels = 0;
  if (tid < NUM_IDS) {
    if (tid >= 1) {
      pid = hdr[tid * ENT + 0];
      uid = hdr[tid * ENT + 1];
      seen = hdr[tid * ENT + 2];
      hits = hdr[tid * ENT + 3];
      pixels = hdr[tid * ENT + 4];
    }
    if (pid == 0 || step - seen > max_lost) pid = uid = seen = hits = pixels = 0;
    const uoc_track t = T[tid];
    const bool vis = tid >= 1 && t.uid != 0 && t.age == 0 && S[tid * SIG + UOC_SIG_PIXELS] > 0;
    s_tuid[tid] = vis ? t.uid : 0;
    s_pid[tid] = pid;
    s_euid[tid] = uid;
    s_seen[tid] = seen;
    s_ent_of[tid] = s_slot_of[tid] = s_newpid[tid] = 0;
    s_anew[tid] = area64(S + tid * SIG);
    s_aold[tid] = area64(esig + tid * SIG);
  }
  if (tid == 0) s_nlist = 0;
  __syncthreads();
  if (tid >= 1 && tid < NUM_IDS && pid != 0 && uid != 0) {   // bound: the visible slot with this entry's uid (uids are unique)
    for (int s = 1; s < NUM_IDS; ++s)
      if (s_tuid[s] == uid) {
        s_slot_of[tid] = s;
        s_ent_of[s] = tid;
      }
  }
  __syncthreads();
  if (tid < NUM_IDS) {
    s_new[tid] = s_tuid[tid] != 0 && s_ent_of[tid] == 0;   // newcomers
    s_lost[tid] = pid != 0 && s_slot_of[tid] == 0;         // lost entries
  }
  __syncthreads();

  // 3. candidates
  for (int i = tid; i < NUM_IDS * NUM_IDS; i += IDENT_THREADS) {
    const int s = i >> 7, e = i & (NUM_IDS - 1);
    if (!s_new[s] || !s_lost[e]) continue;
    const int sim = pair_similarity(S + s * SIG, esig + e * SIG);
    if (sim < q) continue;
    if (r > 0) {
      const unsigned long long as = s_anew[s], ae = s_aold[e], lo = as < ae ? as : ae, hi = as < ae ? ae : as;
      if (lo == 0ull || lo * 256ull < (unsigned long long)r * hi) continue;
    }
    const int at = atomicAdd(&s_nlist, 1);
    if (at < MAX_CAND) s_list[at] = ((unsigned)sim << 14) | (unsigned)(s << 7) | (unsigned)e;
  }
  __syncthreads();

  // 4. greedy rounds by wave 0; every lane ends a round with the same winner, so the matched sets stay in registers.
  //    The order is one 64-bit key: sim, then seen, then the lower entry, then the lower slot.
  if (wave == 0) {
    const int nlist = min(s_nlist, MAX_CAND);
    unsigned long long ms0 = 0ull, ms1 = 0ull, me0 = 0ull, me1 = 0ull;
    for (;;) {
      unsigned long long best = 0ull;
      for (int k = lane; k < nlist; k += 64) {
        const unsigned c = s_list[k];
        const int s = (c >> 7) & (NUM_IDS - 1), e = c & (NUM_IDS - 1);
        if ((((s & 64 ? ms1 : ms0) >> (s & 63)) | ((e & 64 ? me1 : me0) >> (e & 63))) & 1ull) continue;
        const unsigned long long key = ((unsigned long long)(c >> 14) << 45) | ((unsigned long long)(unsigned)s_seen[e] << 14) |
                                       (unsigned long long)((NUM_IDS - 1 - e) << 7) | (unsigned long long)(NUM_IDS - 1 - s);
        best = max(best, key);
      }
      best = wave_max64(best);
      if (best == 0ull) break;   // the same in every lane; a candidate's key has sim >= q >= 1
      const int e = NUM_IDS - 1 - (int)((best >> 7) & (NUM_IDS - 1)), s = NUM_IDS - 1 - (int)(best & (NUM_IDS - 1));
      (s & 64 ? ms1 : ms0) |= 1ull << (s & 63);
      (e & 64 ? me1 : me0) |= 1ull << (e & 63);
      if (lane == 0) {
        s_ent_of[s] = e;
        s_slot_of[e] = s;
        s_euid[e] = s_tuid[s];
      }
    }
  }
  __syncthreads();

  // 5. the newcomers left over, in ascending order, take the free entries in ascending order, then the lost entries
  //    left over in the order of (seen, entry)
  if (tid < NUM_IDS) {
    s_new[tid] = s_tuid[tid] != 0 && s_ent_of[tid] == 0;
    s_lost[tid] = pid != 0 && s_slot_of[tid] == 0;
    s_free[tid] = tid >= 1 && pid == 0;
  }
  __syncthreads();
  int rank_new = 0, n_new = 0, n_free = 0, n_lost = 0;
  if (tid < NUM_IDS) {
    int rank_free = 0, rank_lost = 0;
    for (int j = 1; j < NUM_IDS; ++j) {
      n_new += s_new[j];
      n_free += s_free[j];
      n_lost += s_lost[j];
      if (j < tid) {
        rank_new += s_new[j];
        rank_free += s_free[j];
      }
      if (s_lost[j] && (s_seen[j] < seen || (s_seen[j] == seen && j < tid))) rank_lost += 1;
    }
    if (s_free[tid]) s_free_at[rank_free] = tid;
    if (s_lost[tid]) s_lost_at[rank_lost] = tid;
  }
  __syncthreads();
  if (tid < NUM_IDS && s_new[tid] && rank_new < n_free + n_lost) {   // always true for a tracker's table: 127 entries, 127 slots
    const int e = rank_new < n_free ? s_free_at[rank_new] : s_lost_at[rank_new - n_free];
    s_ent_of[tid] = e;
    s_slot_of[e] = tid;
    s_euid[e] = s_tuid[tid];
    s_newpid[e] = pids + 1 + rank_new;
  }
  __syncthreads();

  // 6. the table, the lut, the counters and the stored signatures
  if (tid < NUM_IDS) {
    if (s_newpid[tid]) {
      pid = s_newpid[tid];
      hits = 0;
    }
    uid = s_euid[tid];
    const int s = s_slot_of[tid];
    if (s) {
      seen = step;
      hits += 1;
      pixels = S[s * SIG + UOC_SIG_PIXELS];
    }
    s_pid[tid] = pid;
    const int rec[ENT] = {pid, uid, seen, hits, pixels};
#pragma unroll
    for (int k = 0; k < ENT; ++k) {
      hdr[tid * ENT + k] = rec[k];
      if (ident_out) ident_out[((size_t)b * NUM_IDS + tid) * ENT + k] = rec[k];
    }
    plan[(size_t)b * NUM_IDS + tid] = s_ent_of[tid];
    if (lut_out) lut_out[(size_t)b * NUM_IDS + tid] = s_ent_of[tid];
  }
  if (tid == 0) {
    const int taken = n_new < n_free + n_lost ? n_new : n_free + n_lost;
    hdr[META + 0] = pids + taken;
    hdr[META + 1] = step;
    hdr[META + 2] = evicted + (taken > n_free ? taken - n_free : 0);
  }
  __syncthreads();
  for (int i = tid; i < NUM_IDS * SIG; i += IDENT_THREADS) {
    const int e = i / SIG, s = s_slot_of[e];
    if (s)
      esig[i] = S[s * SIG + i % SIG];
    else if (s_pid[e] == 0)
      esig[i] = 0;
  }
}

template <int V>
__global__ __launch_bounds__(256) void relabel_kernel(const int *__restrict__ tracked, int n, const int *__restrict__ plan,
                                                      int *__restrict__ out) {
  __shared__ int s_lut[NUM_IDS];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (tid < NUM_IDS) s_lut[tid] = plan[(size_t)b * NUM_IDS + tid];
  __syncthreads();
  const int *L = tracked + (size_t)b * n;
  int *O = out + (size_t)b * n;
  const long long nv = n / V, step = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + tid; i < nv; i += step) {
    if (V == 4) {
      const int4 l = reinterpret_cast<const int4 *>(L)[i];
      reinterpret_cast<int4 *>(O)[i] = make_int4(s_lut[obj_id(l.x)], s_lut[obj_id(l.y)], s_lut[obj_id(l.z)], s_lut[obj_id(l.w)]);
    } else {
      O[i] = s_lut[obj_id(L[i])];
    }
  }
}

inline int pixel_blocks(int n) {
  const int blocks = (n + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK;
  return blocks > MAX_BLOCKS ? MAX_BLOCKS : blocks;
}

}  // namespace
}  // namespace uoc

using namespace uoc;

extern "C" {

size_t uoc_signature_workspace_bytes(int B) {
  if (B <= 0 || B > 65535) return 0;
  return (size_t)B * NUM_IDS * SIG * sizeof(int32_t);
}

int uoc_signature(const int32_t *d_labels, const uint8_t *d_image, const float *d_xyz, int B, int H, int W, int32_t *d_sig,
                  void *d_ws, size_t ws_bytes, void *stream) {
  UOC_REQUIRE(d_labels && d_image && d_sig && d_ws, "uoc_signature: null labels / image / sig / workspace");
  UOC_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "uoc_signature: bad shape B=%d H=%d W=%d", B, H, W);
  UOC_REQUIRE((long long)H * W <= UOC_SIG_MAX_N, "uoc_signature: H*W = %lld above UOC_SIG_MAX_N = %d (a vote counter is 32 bits)",
              (long long)H * W, UOC_SIG_MAX_N);
  UOC_REQUIRE(ws_bytes >= uoc_signature_workspace_bytes(B), "uoc_signature: workspace %zu < %zu bytes", ws_bytes,
              uoc_signature_workspace_bytes(B));
  UOC_REQUIRE((((uintptr_t)d_ws | (uintptr_t)d_sig) & 15) == 0, "uoc_signature: sig / workspace not 16-byte aligned");
  UOC_REQUIRE(((uintptr_t)d_labels & 3) == 0 && (!d_xyz || ((uintptr_t)d_xyz & 3) == 0), "uoc_signature: labels / xyz not 4-byte aligned");
  const int n = H * W;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = n % 4 == 0 && ((uintptr_t)d_labels & 15) == 0 && ((uintptr_t)d_image & 3) == 0 && ((uintptr_t)d_xyz & 15) == 0;
  unsigned *acc = (unsigned *)d_ws;
  if (vec)
    hipLaunchKernelGGL(sig_kernel<4>, dim3(pixel_blocks(n), B), dim3(SIG_THREADS), 0, st, d_labels, d_image, d_xyz, acc, n);
  else
    hipLaunchKernelGGL(sig_kernel<1>, dim3(pixel_blocks(n), B), dim3(SIG_THREADS), 0, st, d_labels, d_image, d_xyz, acc, n);
  hipLaunchKernelGGL(sig_finish, dim3(NUM_IDS, B), dim3(NUM_IDS), 0, st, acc, d_sig);
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

int uoc_sig_similarity(const int32_t *d_sig_a, const int32_t *d_sig_b, int B, int32_t *d_sim, void *stream) {
  UOC_REQUIRE(d_sig_a && d_sig_b && d_sim, "uoc_sig_similarity: null sig_a / sig_b / sim");
  UOC_REQUIRE(B > 0 && B <= 65535, "uoc_sig_similarity: bad B=%d", B);
  UOC_REQUIRE((((uintptr_t)d_sig_a | (uintptr_t)d_sig_b) & 15) == 0, "uoc_sig_similarity: signatures not 16-byte aligned");
  hipLaunchKernelGGL(sim_kernel, dim3(NUM_IDS, B), dim3(NUM_IDS), 0, (hipStream_t)stream, d_sig_a, d_sig_b, d_sim);
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

size_t uoc_ident_state_bytes(int B) {
  if (B <= 0 || B > 65535) return 0;
  return (size_t)B * STATE_WORDS * sizeof(int32_t);
}

size_t uoc_ident_workspace_bytes(int B) {
  if (B <= 0 || B > 65535) return 0;
  return (size_t)B * NUM_IDS * sizeof(int32_t);
}

int uoc_ident_reset(void *d_state, int B, int which, void *stream) {
  UOC_REQUIRE(d_state, "uoc_ident_reset: null state");
  UOC_REQUIRE(B > 0 && B <= 65535, "uoc_ident_reset: bad B=%d", B);
  UOC_REQUIRE(which >= -1 && which < B, "uoc_ident_reset: stream %d outside [-1, %d)", which, B);
  const size_t stride = (size_t)STATE_WORDS * sizeof(int32_t);
  if (which < 0)
    UOC_HIP_CHECK(hipMemsetAsync(d_state, 0, stride * (size_t)B, (hipStream_t)stream));
  else
    UOC_HIP_CHECK(hipMemsetAsync((char *)d_state + stride * (size_t)which, 0, stride, (hipStream_t)stream));
  return UOC_OK;
}

int uoc_ident_step(const int32_t *d_tracked, const uoc_track *d_tracks, const int32_t *d_sig, int B, int H, int W, int q, int r,
                   int max_lost, void *d_state, int32_t *d_out, int32_t *d_lut, int32_t *d_ident, void *d_ws, size_t ws_bytes,
                   void *stream) {
  UOC_REQUIRE(d_tracked && d_tracks && d_sig && d_state && d_out && d_ws,
              "uoc_ident_step: null tracked / tracks / sig / state / out / workspace");
  UOC_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "uoc_ident_step: bad shape B=%d H=%d W=%d", B, H, W);
  UOC_REQUIRE((long long)H * W <= INT_MAX, "uoc_ident_step: H*W = %lld does not fit 31 bits", (long long)H * W);
  UOC_REQUIRE(q >= 1 && q <= 65536, "uoc_ident_step: q = %d outside [1, 65536] (q = round(min_sim * 65536))", q);
  UOC_REQUIRE(r >= 0 && r <= 256, "uoc_ident_step: r = %d outside [0, 256] (r = round(min_size * 256))", r);
  UOC_REQUIRE(max_lost >= 0, "uoc_ident_step: max_lost = %d is negative", max_lost);
  UOC_REQUIRE(ws_bytes >= uoc_ident_workspace_bytes(B), "uoc_ident_step: workspace %zu < %zu bytes", ws_bytes,
              uoc_ident_workspace_bytes(B));
  UOC_REQUIRE((((uintptr_t)d_state | (uintptr_t)d_ws | (uintptr_t)d_sig) & 15) == 0,
              "uoc_ident_step: state / workspace / sig not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)MAX_CAND * sizeof(unsigned);
  static DeviceOnce attr_set;
  if (int rc = opt_in_dynamic_lds(reinterpret_cast<const void *>(&ident_kernel), lds, attr_set)) return rc;
  int *plan = (int *)d_ws;
  hipLaunchKernelGGL(ident_kernel, dim3(B), dim3(IDENT_THREADS), lds, st, d_tracks, d_sig, (int *)d_state, q, r, max_lost, plan,
                     d_lut, d_ident);
  const int n = H * W;
  const bool vec = n % 4 == 0 && (((uintptr_t)d_tracked | (uintptr_t)d_out) & 15) == 0;
  const int blocks = pixel_blocks(n) * 4;   // 256-thread blocks over the same pixels
  if (vec)
    hipLaunchKernelGGL(relabel_kernel<4>, dim3(blocks, B), dim3(256), 0, st, d_tracked, n, plan, d_out);
  else
    hipLaunchKernelGGL(relabel_kernel<1>, dim3(blocks, B), dim3(256), 0, st, d_tracked, n, plan, d_out);
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

}  // extern "C"
