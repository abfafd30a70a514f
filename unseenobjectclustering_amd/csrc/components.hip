// Spatially connected components of a label map (include/uoc_hip.h, uoc_cc_*): the pixels of one id
// that touch each other (4- or 8-connected) form a component; small components become background and the rest are
// renumbered 1..127 in raster order (mode ALL) or cut down to the largest one per raw id (mode LARGEST).  B independent
// frames per call, no host round trip, integer arithmetic only.
//
// Union-find over raster indices i = y*W + x with "the smaller index becomes the parent": whatever the order of the
// unions, a component's root ends up as its smallest raster index.
//
// Workspace per frame (uoc_cc_workspace_bytes / B):
//   int32 [512]   header: sib[128] components per raw id, best[128] as uint64 (area << 32 | ~root, LARGEST), small count
//   int32 [nblk]  surviving roots per 1024-pixel block, then their exclusive scan
//   int32 [H*W]   parent: -1 background, else an index of the same component that is <= the pixel's own
//   int32 [H*W]   cnt: tile-local area at tile-local roots -> area at roots -> new id at roots (ALL)
//
// Launches on grids (block, frame), each phase its own launch (a kernel boundary is what makes the parent array
// visible across the chip):
//   tile_kernel     a 32x32 tile in LDS: unions by atomicMin on a shared parent array, flatten, per-root pixel counts;
//                   writes roots as global raster indices; block 0 zeroes the frame's header
//   merge_kernel    the neighbour pairs that cross a tile border, by atomicMin on the global parent array
//   flatten_kernel  parent[i] = root(i); tile-local areas are added to their root's (integer atomicAdd)
//   stats_kernel    per raw id the number of roots, per block the number of roots with area >= min_area, the count of
//                   small ones and, for LARGEST, atomicMax of (area, ~root) per raw id — LDS first, one flush per block
//   plan_kernel     one block per frame: scan of the per-block counts, counts[b], LARGEST's table (ALL: zeroes it)
//   rank_kernel     ALL only: rank of a surviving root = block base + ballot prefix; new id and table row at the root
//   write_kernel    out from the root's new id (ALL) or the raw id where the root is the id's winner (LARGEST); int4
//                   where H*W and the pointers allow
// Which neighbour pairs are united (p = (y,x) of id c; W, N, NW, NE its left, upper, upper-left, upper-right neighbours;
// "same" = inside the image with id c):  W if same;  N if same and not (W and NW same);  with connectivity 8 also NW if
// same and neither N nor W same, and NE if same and N not same.  The skipped pairs are joined through the others
// (induction along the row), so the partition is that of the full neighbourhood.
#include "labelmap.h"

#include <limits.h>

namespace uoc {
namespace {

constexpr int TW = 32, TH = 32;         // tile of tile_kernel; one thread per pixel
constexpr int TILE_THREADS = TW * TH;
constexpr int PIX_THREADS = 1024;       // pixels per block of the per-pixel kernels
constexpr int HDR_WORDS = 512;          // header words per frame
constexpr int HDR_SIB = 0;              // int32 [128]
constexpr int HDR_BEST = 128;           // uint64 [128] (8-byte aligned: the header is)
constexpr int HDR_SMALL = 384;          // int32: components below min_area

typedef unsigned long long u64;

struct Layout {
  size_t nblk, off_blk, off_parent, off_cnt, stride;   // byte offsets within a frame's workspace
};
inline Layout layout(long long n) {
  Layout l;
  l.nblk = (size_t)((n + PIX_THREADS - 1) / PIX_THREADS);
  l.off_blk = (size_t)HDR_WORDS * 4;
  l.off_parent = align_up(l.off_blk + l.nblk * 4, 16);
  l.off_cnt = align_up(l.off_parent + (size_t)n * 4, 16);
  l.stride = align_up(l.off_cnt + (size_t)n * 4, 256);
  return l;
}
struct Frame {
  int *hdr, *blk, *parent, *cnt;
};
__device__ __forceinline__ Frame frame_of(void *ws, const Layout &l, int b) {
  char *p = (char *)ws + l.stride * b;
  return Frame{(int *)p, (int *)(p + l.off_blk), (int *)(p + l.off_parent), (int *)(p + l.off_cnt)};
}

// ---- union-find in LDS ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(volatile int *par, int i) {
  for (int p; (p = par[i]) != i;) i = p;
  return i;
}
// Every value ever stored in par[a] is a member of a's component that is <= a, so the loop only descends.  When the
// atomicMin finds that `a` had stopped being a root, the pair (its old parent, b) is still to be joined: carry on there.
__device__ __forceinline__ void lds_union(int *par, int a, int b) {
  for (;;) {
    a = lds_find(par, a);
    b = lds_find(par, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&par[a], b);
    if (old == a) return;
    a = old;
  }
}

// ---- 1. tiles -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TILE_THREADS) void tile_kernel(const int *__restrict__ labels, void *__restrict__ ws, Layout lay,
                                                            int H, int W, int tiles_x, int conn8) {
  __shared__ int s_lab[TILE_THREADS], s_par[TILE_THREADS], s_cnt[TILE_THREADS];
  const int tid = threadIdx.x, lx = tid & (TW - 1), ly = tid / TW, b = blockIdx.y;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int x = tx * TW + lx, y = ty * TH + ly;
  const Frame f = frame_of(ws, lay, b);
  if (blockIdx.x == 0 && tid < HDR_WORDS) f.hdr[tid] = 0;
  const bool in = x < W && y < H;
  const long long n = (long long)H * W;
  const int g = in ? y * W + x : 0;
  const int c = in ? obj_id(labels[(size_t)b * n + g]) : 0;
  s_lab[tid] = c;
  s_par[tid] = tid;
  s_cnt[tid] = 0;
  __syncthreads();
  if (c) {   // neighbours outside the tile count as "not same" here: that only adds unions
    const bool w = lx > 0 && s_lab[tid - 1] == c;
    const bool nn = ly > 0 && s_lab[tid - TW] == c;
    const bool nw = lx > 0 && ly > 0 && s_lab[tid - TW - 1] == c;
    const bool ne = lx < TW - 1 && ly > 0 && s_lab[tid - TW + 1] == c;
    if (w) lds_union(s_par, tid, tid - 1);
    if (nn && !(w && nw)) lds_union(s_par, tid, tid - TW);
    if (conn8) {
      if (nw && !nn && !w) lds_union(s_par, tid, tid - TW - 1);
      if (ne && !nn) lds_union(s_par, tid, tid - TW + 1);
    }
  }
  __syncthreads();
  int root = tid;
  if (c) {
    root = lds_find(s_par, tid);
    // the usual case, a wave inside one blob: one add for the wave
    const int first = __builtin_amdgcn_readfirstlane(root);
    const u64 same = __ballot(root == first);
    if (same == __ballot(1)) {
      if (lane_rank(same) == 0) atomicAdd(&s_cnt[root], (int)__popcll(same));
    } else {
      atomicAdd(&s_cnt[root], 1);
    }
  }
  __syncthreads();
  if (in) {
    const int rx = root & (TW - 1), ry = root / TW;
    f.parent[g] = c ? (ty * TH + ry) * W + tx * TW + rx : -1;
    f.cnt[g] = (c && root == tid) ? s_cnt[tid] : 0;
  }
}

// ---- union-find on the global parent array ----------------------------------------------------------------------------
// Other blocks change the array while this one reads it: the loads are agent-scope atomic loads so that none is served
// from a line this CU cached earlier.  A value that is already outdated is still a member of the component.
__device__ __forceinline__ int g_load(int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(int *par, int i) {
  for (int p; (p = g_load(&par[i])) != i;) i = p;
  return i;
}
__device__ __forceinline__ void g_union(int *par, int a, int b) {
  for (;;) {
    a = g_find(par, a);
    b = g_find(par, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&par[a], b);
    if (old == a) return;
    a = old;
  }
}

// ---- 2. tile borders ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PIX_THREADS) void merge_kernel(const int *__restrict__ labels, void *__restrict__ ws, Layout lay,
                                                            int H, int W, int conn8) {
  const int b = blockIdx.y;
  const long long n = (long long)H * W, i = (long long)blockIdx.x * PIX_THREADS + threadIdx.x;
  if (i >= n) return;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  const int lx = x & (TW - 1), ly = y & (TH - 1);
  if (lx != 0 && ly != 0 && !(conn8 && lx == TW - 1)) return;   // no neighbour of this pixel lies in another tile
  const int *L = labels + (size_t)b * n;
  const int c = obj_id(L[i]);
  if (!c) return;
  const Frame f = frame_of(ws, lay, b);
  const bool w = x > 0 && obj_id(L[i - 1]) == c;
  const bool nn = y > 0 && obj_id(L[i - W]) == c;
  const bool nw = x > 0 && y > 0 && obj_id(L[i - W - 1]) == c;
  const bool ne = x < W - 1 && y > 0 && obj_id(L[i - W + 1]) == c;
  const int p = (int)i;
  if (w && lx == 0) g_union(f.parent, p, p - 1);
  if (nn && ly == 0 && !(w && nw)) g_union(f.parent, p, p - W);
  if (conn8) {
    if (nw && !nn && !w && (lx == 0 || ly == 0)) g_union(f.parent, p, p - W - 1);
    if (ne && !nn && (lx == TW - 1 || ly == 0)) g_union(f.parent, p, p - W + 1);
  }
}

// ---- 3. flatten, areas ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PIX_THREADS) void flatten_kernel(void *__restrict__ ws, Layout lay, long long n) {
  const long long i = (long long)blockIdx.x * PIX_THREADS + threadIdx.x;
  if (i >= n) return;
  const Frame f = frame_of(ws, lay, blockIdx.y);
  int p = f.parent[i];
  if (p < 0 || p == (int)i) return;
  for (int q; (q = f.parent[p]) != p;) p = q;   // concurrent writers only store roots: still an ancestor
  f.parent[i] = p;
  const int a = f.cnt[i];   // non-zero at the roots the tiles found; nothing is ever added to a pixel that is not a final root
  if (a) atomicAdd(&f.cnt[p], a);
}

// ---- 4. per-id and per-block statistics -------------------------------------------------------------------------------------
template <bool LARGEST>
__global__ __launch_bounds__(PIX_THREADS) void stats_kernel(const int *__restrict__ labels, void *__restrict__ ws, Layout lay,
                                                            long long n, int min_area) {
  __shared__ int s_sib[NUM_IDS], s_small, s_surv;
  __shared__ u64 s_best[NUM_IDS];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (tid < NUM_IDS) {
    s_sib[tid] = 0;
    s_best[tid] = 0ull;
  }
  if (tid == 0) s_small = s_surv = 0;
  __syncthreads();
  const Frame f = frame_of(ws, lay, b);
  const long long i = (long long)blockIdx.x * PIX_THREADS + tid;
  const bool root = i < n && f.parent[i] == (int)i;
  int area = 0;
  if (root) {
    area = f.cnt[i];
    const int c = obj_id(labels[(size_t)b * n + i]);
    atomicAdd(&s_sib[c], 1);
    if (LARGEST && area >= min_area) atomicMax(&s_best[c], ((u64)(unsigned)area << 32) | (unsigned)~(unsigned)i);
  }
  const u64 small = __ballot(root && area < min_area), surv = __ballot(root && area >= min_area);
  if ((tid & 63) == 0) {
    if (small) atomicAdd(&s_small, (int)__popcll(small));
    if (surv) atomicAdd(&s_surv, (int)__popcll(surv));
  }
  __syncthreads();
  if (tid < NUM_IDS) {
    if (s_sib[tid]) atomicAdd(&f.hdr[HDR_SIB + tid], s_sib[tid]);
    if (LARGEST && s_best[tid]) atomicMax(reinterpret_cast<u64 *>(f.hdr + HDR_BEST) + tid, s_best[tid]);
  }
  if (tid == 0) {
    f.blk[blockIdx.x] = s_surv;
    if (s_small) atomicAdd(&f.hdr[HDR_SMALL], s_small);
  }
}

// ---- 5. plan: block bases, counts, LARGEST's table ----------------------------------------------------------------------------
__global__ __launch_bounds__(PIX_THREADS) void plan_kernel(void *__restrict__ ws, Layout lay, int largest,
                                                           int *__restrict__ table, int *__restrict__ counts) {
  __shared__ int s_scan[PIX_THREADS], s_found[NUM_IDS], s_kept[NUM_IDS];
  const int tid = threadIdx.x, b = blockIdx.x;
  const Frame f = frame_of(ws, lay, b);
  // exclusive scan of the per-block counts: a contiguous segment per thread, then a scan of the segment sums
  const size_t per = (lay.nblk + PIX_THREADS - 1) / PIX_THREADS;
  const size_t lo = (size_t)tid * per, hi = lo + per < lay.nblk ? lo + per : lay.nblk;
  int sum = 0;
  for (size_t k = lo; k < hi; ++k) sum += f.blk[k];
  s_scan[tid] = sum;
  __syncthreads();
  for (int d = 1; d < PIX_THREADS; d <<= 1) {
    const int v = tid >= d ? s_scan[tid - d] : 0;
    __syncthreads();
    s_scan[tid] += v;
    __syncthreads();
  }
  const int total = s_scan[PIX_THREADS - 1];
  int run = s_scan[tid] - sum;
  for (size_t k = lo; k < hi; ++k) {
    const int v = f.blk[k];
    f.blk[k] = run;
    run += v;
  }
  int *T = table + (size_t)b * NUM_IDS * 4;
  if (tid < NUM_IDS) {
    const int sib = tid ? f.hdr[HDR_SIB + tid] : 0;
    s_found[tid] = sib;
    int4 row = make_int4(0, 0, 0, 0);
    int kept = 0;
    if (largest && tid) {
      const u64 best = reinterpret_cast<const u64 *>(f.hdr + HDR_BEST)[tid];
      if (best) {
        row = make_int4(tid, (int)(best >> 32), (int)~(unsigned)best, sib);
        kept = 1;
      }
    }
    s_kept[tid] = kept;
    reinterpret_cast<int4 *>(T)[tid] = row;   // ALL: zeroed here, rank_kernel fills the used rows
  }
  __syncthreads();
  if (tid == 0) {
    int found = 0, kept = 0;
    for (int k = 1; k < NUM_IDS; ++k) {
      found += s_found[k];
      kept += s_kept[k];
    }
    if (!largest) kept = total < NUM_IDS - 1 ? total : NUM_IDS - 1;
    int *C = counts + (size_t)b * 4;
    C[0] = found;
    C[1] = f.hdr[HDR_SMALL];
    C[2] = kept;
    C[3] = total - kept;
  }
}

// ---- 6. ALL: raster rank of the surviving roots --------------------------------------------------------------------------------
__global__ __launch_bounds__(PIX_THREADS) void rank_kernel(const int *__restrict__ labels, void *__restrict__ ws, Layout lay,
                                                           long long n, int min_area, int *__restrict__ table) {
  __shared__ int s_wave[PIX_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
  const Frame f = frame_of(ws, lay, b);
  const long long i = (long long)blockIdx.x * PIX_THREADS + tid;
  const bool root = i < n && f.parent[i] == (int)i;
  const int area = root ? f.cnt[i] : 0;
  const bool surv = root && area >= min_area;
  const u64 bal = __ballot(surv);
  if (lane == 0) s_wave[wave] = (int)__popcll(bal);
  __syncthreads();
  if (!root) return;
  int id = 0;
  if (surv) {
    int rank = f.blk[blockIdx.x] + lane_rank(bal);
    for (int k = 0; k < wave; ++k) rank += s_wave[k];
    if (rank < NUM_IDS - 1) {
      id = rank + 1;
      const int c = obj_id(labels[(size_t)b * n + i]);
      reinterpret_cast<int4 *>(table + (size_t)b * NUM_IDS * 4)[id] = make_int4(c, area, (int)i, f.hdr[HDR_SIB + c]);
    }
  }
  f.cnt[i] = id;
}

// ---- 7. the output map ---------------------------------------------------------------------------------------------------------
template <int V, bool LARGEST>
__global__ __launch_bounds__(256) void write_kernel(const int *__restrict__ labels, void *__restrict__ ws, Layout lay,
                                                    long long n, int *__restrict__ out) {
  __shared__ int s_win[NUM_IDS];   // LARGEST: root of the id's winner
  const int tid = threadIdx.x, b = blockIdx.y;
  const Frame f = frame_of(ws, lay, b);
  if (LARGEST) {
    if (tid < NUM_IDS) {
      const u64 best = reinterpret_cast<const u64 *>(f.hdr + HDR_BEST)[tid];
      s_win[tid] = (tid && best) ? (int)~(unsigned)best : -2;
    }
    __syncthreads();
  }
  const int *L = labels + (size_t)b * n;
  int *O = out + (size_t)b * n;
  auto one = [&](int l, int p) -> int {
    if (LARGEST) {
      const int c = obj_id(l);
      return s_win[c] == p ? c : 0;
    }
    return p >= 0 ? f.cnt[p] : 0;
  };
  const long long nv = n / V, step = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + tid; i < nv; i += step) {
    if (V == 4) {
      const int4 p = reinterpret_cast<const int4 *>(f.parent)[i];
      int4 l = make_int4(0, 0, 0, 0);
      if (LARGEST) l = reinterpret_cast<const int4 *>(L)[i];
      reinterpret_cast<int4 *>(O)[i] = make_int4(one(l.x, p.x), one(l.y, p.y), one(l.z, p.z), one(l.w, p.w));
    } else {
      O[i] = one(LARGEST ? L[i] : 0, f.parent[i]);
    }
  }
}

inline bool shape_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && (long long)H * W <= INT_MAX; }

}  // namespace
}  // namespace uoc

using namespace uoc;

extern "C" {

size_t uoc_cc_workspace_bytes(int B, int H, int W) {
  if (!shape_ok(B, H, W)) return 0;
  return layout((long long)H * W).stride * (size_t)B;
}

int uoc_cc_split(const int32_t *d_labels, int B, int H, int W, int connectivity, int min_area, int mode, int32_t *d_out,
                 int32_t *d_table, int32_t *d_counts, void *d_ws, size_t ws_bytes, void *stream) {
  UOC_REQUIRE(d_labels && d_out && d_table && d_counts && d_ws, "uoc_cc_split: null labels / out / table / counts / workspace");
  UOC_REQUIRE(d_out != d_labels, "uoc_cc_split: out must not alias labels");
  UOC_REQUIRE(shape_ok(B, H, W), "uoc_cc_split: bad shape B=%d H=%d W=%d (H*W must be below 2^31)", B, H, W);
  UOC_REQUIRE(connectivity == 4 || connectivity == 8, "uoc_cc_split: connectivity = %d is neither 4 nor 8", connectivity);
  UOC_REQUIRE(min_area >= 1, "uoc_cc_split: min_area = %d below 1", min_area);
  UOC_REQUIRE(mode == UOC_CC_ALL || mode == UOC_CC_LARGEST, "uoc_cc_split: unknown mode %d", mode);
  UOC_REQUIRE(ws_bytes >= uoc_cc_workspace_bytes(B, H, W), "uoc_cc_split: workspace %zu < %zu bytes", ws_bytes,
              uoc_cc_workspace_bytes(B, H, W));
  UOC_REQUIRE((((uintptr_t)d_ws | (uintptr_t)d_table) & 15) == 0, "uoc_cc_split: workspace / table not 16-byte aligned");
  const long long n = (long long)H * W;
  const Layout lay = layout(n);
  hipStream_t st = (hipStream_t)stream;
  const int conn8 = connectivity == 8, largest = mode == UOC_CC_LARGEST;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const dim3 pix((unsigned)lay.nblk, B);
  hipLaunchKernelGGL(tile_kernel, dim3(tiles_x * tiles_y, B), dim3(TILE_THREADS), 0, st, d_labels, d_ws, lay, H, W, tiles_x, conn8);
  if (tiles_x * tiles_y > 1)
    hipLaunchKernelGGL(merge_kernel, pix, dim3(PIX_THREADS), 0, st, d_labels, d_ws, lay, H, W, conn8);
  hipLaunchKernelGGL(flatten_kernel, pix, dim3(PIX_THREADS), 0, st, d_ws, lay, n);
  if (largest)
    hipLaunchKernelGGL(stats_kernel<true>, pix, dim3(PIX_THREADS), 0, st, d_labels, d_ws, lay, n, min_area);
  else
    hipLaunchKernelGGL(stats_kernel<false>, pix, dim3(PIX_THREADS), 0, st, d_labels, d_ws, lay, n, min_area);
  hipLaunchKernelGGL(plan_kernel, dim3(B), dim3(PIX_THREADS), 0, st, d_ws, lay, largest, d_table, d_counts);
  if (!largest)
    hipLaunchKernelGGL(rank_kernel, pix, dim3(PIX_THREADS), 0, st, d_labels, d_ws, lay, n, min_area, d_table);
  const bool vec = n % 4 == 0 && (((uintptr_t)d_labels | (uintptr_t)d_out) & 15) == 0;
  const long long items = vec ? n / 4 : n;
  long long wb = (items + 255) / 256;
  if (wb > 4096) wb = 4096;   // grid-stride beyond
  const dim3 wgrid((unsigned)wb, B);
  if (vec && largest)
    hipLaunchKernelGGL((write_kernel<4, true>), wgrid, dim3(256), 0, st, d_labels, d_ws, lay, n, d_out);
  else if (vec)
    hipLaunchKernelGGL((write_kernel<4, false>), wgrid, dim3(256), 0, st, d_labels, d_ws, lay, n, d_out);
  else if (largest)
    hipLaunchKernelGGL((write_kernel<1, true>), wgrid, dim3(256), 0, st, d_labels, d_ws, lay, n, d_out);
  else
    hipLaunchKernelGGL((write_kernel<1, false>), wgrid, dim3(256), 0, st, d_labels, d_ws, lay, n, d_out);
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

}  // extern "C"
