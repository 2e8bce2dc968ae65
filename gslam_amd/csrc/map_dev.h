// The device-side pieces that the map stages share: gh_link_tracks_dev (track_link.hip), gh_extend_tracks_dev (track_extend.hip),
// gh_merge_points_dev (track_merge.hip), gh_pnp_gather_pairs_dev / gh_localize_pairs_dev (localize.hip) and gh_ba_window_dev
// (ba_window.hip); gh_ransac_pairs_dev (ransac_batch.hip) takes the pinhole from here, gh_describe_points_dev (point_describe.hip)
// and gh_search_projection_dev (search_projection.hip) the spare bins, the scale table and the Hamming distance.  Everything is
// __device__ __forceinline__: a kernel that calls one of these compiles to what it was with the lines written out.  The host-side
// pieces of the same stages are in map_host.h.
#pragma once
#include "common.h"

namespace gh_map {

constexpr int kBlock = 256;
constexpr int kMaxFlagBlocks = 1024;  // the *_flags kernels go grid-stride beyond this many workgroups

// the rows of frame f that exist: counts[f] clamped to [0, cap]
__device__ __forceinline__ int row_count(const int32_t* __restrict__ counts, int f, int cap) {
  const int c = counts[f];
  return c < 0 ? 0 : (c > cap ? cap : c);
}

struct PairRows {
  const int32_t* counts;
  int n_frames, cap;
  const int32_t* pair_q;
  const int32_t* pair_t;
  const int32_t* idx1;
  const uint8_t* keep;  // may be NULL: every row is kept
};

// THE EDGE RULE, the gather rule of gh_ransac_pairs_dev: row r = p * cap + i of the pair arrays is an edge when both frames of
// pair p are in range and differ, query row i exists in frame pair_q[p], keep[r] (if given) is not zero and
// 0 <= idx1[r] < the rows of frame pair_t[p].  *u and *v are the two node ids, frame * cap + row, query end first.  What a stage
// does with the edge is the stage's own.
__device__ __forceinline__ bool pair_edge(const PairRows& e, long long r, int* u, int* v) {
  const int p = (int)(r / e.cap), i = (int)(r - (long long)p * e.cap);
  const int fq = e.pair_q[p], ft = e.pair_t[p];
  if (fq < 0 || fq >= e.n_frames || ft < 0 || ft >= e.n_frames || fq == ft) return false;
  if (i >= row_count(e.counts, fq, e.cap)) return false;
  if (e.keep && e.keep[r] == 0) return false;
  const int j = e.idx1[r];
  if (j < 0 || j >= row_count(e.counts, ft, e.cap)) return false;
  *u = fq * e.cap + i;
  *v = ft * e.cap + j;
  return true;
}

// words[key] += 1 for every lane that is `on`, exactly, with one atomic per RUN of neighbouring lanes that share the key: they
// fold their ones into the first of them (a ballot and a bit scan).  Every lane of the wave must call it (on = false where a
// lane has nothing to add).
__device__ __forceinline__ void add_runs(int32_t* words, int key, bool on) {
  const int lane = threadIdx.x & 63;
  const int prev_key = __shfl_up(key, 1);
  const unsigned long long on_mask = __ballot(on);
  const bool prev_on = lane > 0 && ((on_mask >> (lane - 1)) & 1ull) != 0;
  const bool head = on && (!prev_on || prev_key != key);
  const unsigned long long stops = __ballot(head || !on);  // the lanes at which a run cannot go on
  if (head) {
    const unsigned long long above = lane == 63 ? 0ull : stops >> (lane + 1);
    atomicAdd(words + key, above ? __ffsll(above) : 64 - lane);
  }
}

// the number of lanes of the wave for which `on` holds: the same value in every lane
__device__ __forceinline__ int wave_count(bool on) { return __popcll(__ballot(on)); }

// The tail of a kernel that counts K kinds of things: n[k] is this WAVE's count of kind k (the same in every lane: wave_count),
// the word dst(k) receives the workgroup's sum.  Lane 0 of each wave adds into LDS, then lane k issues the global integer atomic
// of counter k -- none for a zero count, which is why a workgroup with nothing to report costs nothing.  The K atomics are ONE
// instruction: the counters of a call share a cache line that every workgroup hits, and a request per counter was measured to
// cost loc_flags 7 us of 21 at 1024 workgroups (profiles/map_shared.txt).  It contains barriers: EVERY thread of the workgroup
// must reach it, once per kernel.
template <int K, class Dst>
__device__ __forceinline__ void block_counts_add(const int (&n)[K], Dst dst) {
  static_assert(K >= 1 && K <= 5, "one LDS word and one lane per counter");
  __shared__ int s_count[K];
  if (threadIdx.x < K) s_count[threadIdx.x] = 0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (n[k]) atomicAdd(&s_count[k], n[k]);
  }
  __syncthreads();
  if (threadIdx.x < K && s_count[threadIdx.x]) atomicAdd(dst(threadIdx.x), s_count[threadIdx.x]);
}
// counter k goes to first[k]
template <int K>
__device__ __forceinline__ void block_counts_add(const int (&n)[K], int32_t* first) {
  block_counts_add<K>(n, [first](int k) { return first + k; });
}

// THE SPARE BINS.  A stage that indexes its items by key (gh_csr_index_dev) gives the items that are not indexed -- the padding
// of a map's arrays, mostly -- a key past the real ones, and the index counts its keys with one atomic each: 1.7 M of them on one
// extra bin took 19.8 ms of a 20.4 ms gh_describe_points_dev.  Spread over kSpareBins bins by the item's own
// index they are neighbours' atomics on neighbouring words.  mask is spare_bins(..) - 1 (map_host.h): a power of two less one.
constexpr int kSpareBins = 4096;
__device__ __forceinline__ int spare_key(int first_spare, int i, int mask) { return first_spare + (i & mask); }

// v[l] = scale_factor^l for the levels of an image pyramid (scale_powers, map_host.h, builds it); a kernel takes it by value
constexpr int kMaxLevels = 32;
struct ScalePowers {
  double v[kMaxLevels];
};

// the Hamming distance of two 256-bit descriptors held as 8 words
__device__ __forceinline__ int hamming256(const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  int d = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) d += __popc(a[w] ^ b[w]);
  return d;
}

struct Pinhole {
  double fx, fy, cx, cy;
};

// pixel -> normalised image coordinates: the float widened (exact), one subtraction, one division
__device__ __forceinline__ void normalised_xy(const gh_keypoint& kp, const Pinhole& k, double* xy) {
  xy[0] = ((double)kp.x - k.cx) / k.fx;
  xy[1] = ((double)kp.y - k.cy) / k.fy;
}

// The verdict on the component with label l (link and extend): CONFLICT when two of its nodes share a frame, SHORT when it has
// fewer than min_views nodes, otherwise a track.  A SHORT component enters the totals only from two nodes up: a row that
// nothing matched is not a failed track.
enum Verdict { kConflict, kShort, kTrack };
struct Component {
  int size;
  Verdict verdict;
  __device__ __forceinline__ bool counted_short() const { return verdict == kShort && size >= 2; }
};
__device__ __forceinline__ Component component_verdict(int l, const int32_t* __restrict__ begin, const int32_t* __restrict__ end,
                                                       const uint8_t* __restrict__ conflict, int min_views) {
  const int size = end[l] - begin[l];
  return {size, conflict[l] != 0 ? kConflict : (size < min_views ? kShort : kTrack)};
}

// the observation list that link and extend write: n_obs entries in use, padded to the node count
struct ObsOut {
  int32_t* cam;
  int32_t* point;
  double* xy;
  int32_t* node;
};

// the observation of `node` (a row of frame `cam`) at its rank k
__device__ __forceinline__ void emit_obs(const ObsOut& o, int k, int cam, int point, int node, const gh_keypoint& kp, const Pinhole& pin) {
  o.cam[k] = cam;
  o.point[k] = point;
  o.node[k] = node;
  normalised_xy(kp, pin, o.xy + 2 * (size_t)k);
}

// entry n past n_obs; the entries below n_obs are written by the nodes that own them
__device__ __forceinline__ void pad_obs(const ObsOut& o, int n) {
  o.cam[n] = -1;
  o.point[n] = -1;
  o.node[n] = -1;
  o.xy[2 * (size_t)n] = 0.0;
  o.xy[2 * (size_t)n + 1] = 0.0;
}

}  // namespace gh_map
