// 3-D skeletonisation by thinning on the device: Lee, Kashyap and Chu (1994) with the border order and
// raster-order re-check of the common implementations; equality with skimage has not been checked.
//
// Reference (CPU): skimage.morphology.skeletonize_3d(label) at ske_and_parse.py:83,115,149, weight_br.py:128, prediction.py:127.
// The definition this file implements is written out in DESIGN.md 3d and, executably, in tests/skeleton_oracle.py:
//   pass = six sub-iterations over the border directions 4, 3, 2, 1, 5, 6; repeat until a pass deletes nothing.
//   sub-iteration d: (1) every voxel in parallel on the image as it stands: candidate = foreground, d-neighbour background, not
//   exactly one foreground 26-neighbour, Euler characteristic unchanged by its removal, foreground 26-neighbours form exactly one
//   26-connected component; (2) the candidates in raster order: delete iff the one-component test still holds on the image with
//   the deletions made so far.
//
// Storage: the padded form of the bit-packed volume (bitvol.h): 64 voxels of a row per word, with one zero
// row on each side of axes 0 and 1 and one zero word on each side of a row, so that no neighbour access needs a bounds test.
// One wavefront works on one word, one lane per voxel.  The 27 words around a word are fetched by 27 lanes with one vector load
// and handed round with v_readlane; the 3 x 3 x 3 neighbourhood of a lane is 27 bits, bit (di+1)*9 + (dj+1)*3 + (dk+1).
//
// The raster-order re-check is resolved in rounds.  A candidate's outcome depends only on the candidates among its 13
// raster-earlier neighbours; its later neighbours cannot be decided before it is, so they still show the image at the start of
// the sub-iteration, which is what the sequential scan would see.  A candidate is decided once none of those 13 is an undecided
// candidate.  Candidates decided at the same time are never 26-adjacent, so the bits a round reads are not the bits it writes,
// and the undecided masks are double-buffered: a round reads the previous round's mask only.  Within a round the wavefront
// follows the chains along its own word in registers (recheck_word), so rounds count words and rows, not voxels.  The first
// kRoundLaunches rounds are one launch each over the compacted list of words that hold candidates (chip-wide parallelism while
// most candidates are still open); one workgroup then loops over what is left with a barrier per round, like dti_sweep_kernel
// walks its wavefront.  No kernel waits for another workgroup.  Nothing depends on the order of the compacted list (filled with
// an atomic counter), so the result is deterministic.
#include "volume.h"
#include <algorithm>

namespace seunet {

namespace {

constexpr int kRoundLaunches = 32;   // re-check rounds run as grid-wide launches before the single-workgroup loop
constexpr unsigned kCentre = 1u << 13;

struct SkelTables {
  unsigned adj[27];     // 26-neighbours of cell b inside the 3x3x3 block, centre excluded
  unsigned octant[8];   // the 7 other cubes at a vertex of the centre cube
  unsigned edge[12];    // the 3 other cubes at an edge of the centre cube
  unsigned face[6];     // the cube across a face; face[d - 1] is also the neighbour that border direction d asks to be background
};

constexpr int cell(int i, int j, int k) { return i * 9 + j * 3 + k; }
constexpr int iabs(int v) { return v < 0 ? -v : v; }

constexpr SkelTables make_tables() {
  SkelTables t{};
  for (int a = 0; a < 27; ++a)
    for (int b = 0; b < 27; ++b) {
      const int di = iabs(a / 9 - b / 9), dj = iabs(a / 3 % 3 - b / 3 % 3), dk = iabs(a % 3 - b % 3);
      if (a != b && a != 13 && b != 13 && di <= 1 && dj <= 1 && dk <= 1) t.adj[a] |= 1u << b;
    }
  for (int v = 0; v < 8; ++v)
    for (int o = 0; o < 8; ++o) {
      const int c = cell((v >> 2) + (o >> 2), ((v >> 1) & 1) + ((o >> 1) & 1), (v & 1) + (o & 1));
      if (c != 13) t.octant[v] |= 1u << c;
    }
  for (int axis = 0; axis < 3; ++axis)
    for (int e = 0; e < 4; ++e)
      for (int o = 0; o < 4; ++o) {
        const int p = (e >> 1) + (o >> 1), q = (e & 1) + (o & 1);
        const int c = axis == 0 ? cell(1, p, q) : (axis == 1 ? cell(p, 1, q) : cell(p, q, 1));
        if (c != 13) t.edge[axis * 4 + e] |= 1u << c;
      }
  // directions 1..6: (0,0,-1) (0,0,+1) (0,+1,0) (0,-1,0) (+1,0,0) (-1,0,0)
  t.face[0] = 1u << cell(1, 1, 0); t.face[1] = 1u << cell(1, 1, 2); t.face[2] = 1u << cell(1, 2, 1);
  t.face[3] = 1u << cell(1, 0, 1); t.face[4] = 1u << cell(2, 1, 1); t.face[5] = 1u << cell(0, 1, 1);
  return t;
}

constexpr SkelTables kHostTables = make_tables();
__constant__ SkelTables kTables = make_tables();

struct SkelCtl {              // zeroed before every pass, read back after it
  int changed[6];             // sub-iteration s of the pass deleted a voxel
  unsigned count[6];          // words with candidates in sub-iteration s
  int stuck;                  // the single-workgroup loop gave up (cannot happen: every round decides a candidate)
  int pad[3];
};

// Device-scope loads and stores on the vector path: words written by other wavefronts of the same launch are read again in
// later rounds of the single-workgroup loop, so they must come neither from the scalar cache nor from a stale L1 line.
__device__ __forceinline__ u64 ld(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// lane t < 27 fetches the word at (row t / 3 of the 3x3 rows around the word, word t % 3 - 1); the other lanes fetch nothing
__device__ __forceinline__ u64 fetch_block(const u64* a, long long p, const BitGeom& g, int lane, int lanes) {
  if (lane >= lanes) return 0;
  const int r = lane / 3, c = lane % 3;
  return ld(a + p + (r / 3 - 1) * g.plane_stride * g.row_stride + (r % 3 - 1) * g.row_stride + (c - 1));
}

template <int SRC> __device__ __forceinline__ u64 from_lane(u64 v) {
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, SRC), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), SRC);
  return ((u64)hi << 32) | lo;
}

// the voxels lane - 1, lane, lane + 1 of a row given its previous, own and next word
__device__ __forceinline__ unsigned window3(u64 prev, u64 cur, u64 next, int lane) {
  const u64 lo = (cur << 1) | (prev >> 63);                // bit b = voxel b - 1
  const u64 hi = (cur >> 63) | ((next & 1ull) << 1);       // voxels 63 and 64
  const u64 v = lane == 0 ? lo : ((lo >> lane) | (hi << (64 - lane)));
  return (unsigned)v & 7u;
}

template <int R> struct RowBits {
  static __device__ __forceinline__ unsigned get(u64 mine, int lane) {
    const unsigned here = window3(from_lane<3 * (R - 1)>(mine), from_lane<3 * (R - 1) + 1>(mine), from_lane<3 * (R - 1) + 2>(mine), lane)
                          << (3 * (R - 1));
    return here | RowBits<R - 1>::get(mine, lane);
  }
};
template <> struct RowBits<0> {
  static __device__ __forceinline__ unsigned get(u64, int) { return 0u; }
};

// the 27-bit neighbourhood of this lane's voxel from the first ROWS rows of a fetched block (all lanes of the wave must call)
template <int ROWS> __device__ __forceinline__ unsigned neighbourhood(u64 mine, int lane) { return RowBits<ROWS>::get(mine, lane); }

// (d): the cells of the centre cube that no other cube of the neighbourhood touches leave the Euler characteristic alone
__device__ __forceinline__ bool euler_unchanged(unsigned nb) {
  int dv = 0, de = 0, df = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) dv += (nb & kTables.octant[q]) == 0u;
#pragma unroll
  for (int q = 0; q < 12; ++q) de += (nb & kTables.edge[q]) == 0u;
#pragma unroll
  for (int q = 0; q < 6; ++q) df += (nb & kTables.face[q]) == 0u;
  return dv - de + df - 1 == 0;
}

// (e): the foreground of the 26 neighbours is exactly one 26-connected component (flood fill from its lowest cell)
__device__ __forceinline__ bool one_component(unsigned nb) {
  nb &= ~kCentre;
  if (nb == 0u) return false;
  unsigned comp = nb & (0u - nb), front = comp;
  while (front) {
    const int b = __builtin_ctz(front);
    front &= front - 1u;
    const unsigned add = kTables.adj[b] & nb & ~comp;
    comp |= add;
    front |= add;
  }
  return comp == nb;
}

// step 1 of a sub-iteration: the candidate mask of every word into BOTH undecided buffers, the words that have candidates into
// the list.  `border` = the neighbourhood bit that must be background.
__global__ void __launch_bounds__(256)
skel_candidates_kernel(const u64* __restrict__ bits, BitGeom g, unsigned border, u64* __restrict__ und0, u64* __restrict__ und1,
                       unsigned* __restrict__ list, unsigned* __restrict__ count) {
  const long long t = (blockIdx.x * 256ll + threadIdx.x) >> 6;
  if (t >= g.words) return;                                  // whole wavefronts leave together
  const int lane = threadIdx.x & 63;
  const long long p = word_index(g, t);
  u64 cand = 0;
  if (bits[p] != 0ull) {                                     // uniform; most words of a volume are empty
    const unsigned nb = neighbourhood<9>(fetch_block(bits, p, g, lane, 27), lane);
    bool c = (nb & kCentre) && !(nb & border);
    if (c) {
      const unsigned around = nb & ~kCentre;
      c = __popc(around) != 1 && euler_unchanged(around) && one_component(around);
    }
    cand = __ballot(c);
  }
  if (lane == 0) {
    und0[p] = cand;
    und1[p] = cand;
    if (cand) list[atomicAdd(count, 1u)] = (unsigned)p;
  }
}

// One re-check round on one word.  A candidate is eligible when none of its 12 raster-earlier neighbours in OTHER rows (and, for
// voxel 0, the last voxel of the previous word) is still undecided in `prev`.  The 13th, the voxel before it in its own word,
// is resolved here: the wavefront walks the chains along the word in registers, deciding in each step the eligible candidates
// whose predecessor is no longer open, so a run of candidates along the contiguous axis costs one round per word, not one per
// voxel.  Two candidates decided in one step are never adjacent; the eight other rows do not change where an eligible candidate
// looks.  Deletes the decided candidates whose neighbours still form one component and writes the word's remaining undecided
// mask to `next`.  Returns that mask.  All 64 lanes call; every mask below is uniform.
__device__ __forceinline__ u64 recheck_word(u64* bits, const u64* prev, u64* next, long long p, const BitGeom& g, int lane,
                                            int* changed) {
  const u64 mine = fetch_block(prev, p, g, lane, 14);        // rows (-1,-1) (-1,0) (-1,+1) (0,-1) and the own row's words -1, 0
  const u64 own = from_lane<13>(mine);
  if (own == 0ull) {
    if (lane == 0) st(next + p, 0ull);
    return 0ull;
  }
  const unsigned earlier = neighbourhood<4>(mine, lane);
  const u64 own_prev = from_lane<12>(mine);
  const bool blocked = earlier != 0u || (lane == 0 && (own_prev >> 63) != 0ull);
  const u64 eligible = own & ~__ballot(blocked);
  u64 open = own;
  u64 ready = eligible & ~(open << 1);
  if (ready) {
    const u64 img = fetch_block(bits, p, g, lane, 27);
    const unsigned other_rows = neighbourhood<9>(img, lane) & ~(7u << 12);
    const u64 word_before = from_lane<12>(img), word_after = from_lane<14>(img), word_in = from_lane<13>(img);
    u64 word = word_in;
    do {
      const unsigned nb = other_rows | (window3(word_before, word, word_after, lane) << 12);
      word &= ~__ballot(((ready >> lane) & 1ull) && one_component(nb));
      open &= ~ready;
      ready = eligible & open & ~(open << 1);
    } while (ready);
    if (lane == 0 && word != word_in) {
      st(bits + p, word);
      *changed = 1;
    }
  }
  if (lane == 0) st(next + p, open);
  return open;
}

__global__ void __launch_bounds__(256)
skel_round_kernel(u64* bits, const u64* prev, u64* next, const unsigned* __restrict__ list, const unsigned* __restrict__ count,
                  BitGeom g, int* changed) {
  const unsigned n = *count;
  const int lane = threadIdx.x & 63;
  const unsigned waves = gridDim.x * 4u;
  for (unsigned i = (blockIdx.x * 256u + threadIdx.x) >> 6; i < n; i += waves) recheck_word(bits, prev, next, list[i], g, lane, changed);
}

// The rounds that are left, in one workgroup: compact the words that still hold undecided candidates, then one barrier per
// round.  `und_a` holds the current masks.  Every round decides at least the raster-first open candidate, so the loop ends
// after at most 64 * (open words) rounds; the bound is enforced, and `stuck` reports a violation instead of hanging the card.
__global__ void __launch_bounds__(1024)
skel_finish_kernel(u64* bits, u64* und_a, u64* und_b, const unsigned* __restrict__ list, unsigned* open_list,
                   const unsigned* __restrict__ count, BitGeom g, int* changed, int* stuck) {
  __shared__ unsigned n_open;
  __shared__ int remaining;
  const unsigned n = *count;
  const int lane = threadIdx.x & 63;
  const unsigned wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) n_open = 0u;
  __syncthreads();
  for (unsigned i = wave; i < n; i += 16u) {
    const unsigned p = list[i];
    if (lane == 0 && ld(und_a + p) != 0ull)
      __hip_atomic_store(open_list + atomicAdd(&n_open, 1u), p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const unsigned m = n_open;
  if (m == 0u) return;
  const u64 max_rounds = 64ull * m + 1ull;
  u64* prev = und_a;
  u64* next = und_b;
  for (u64 round = 0;; ++round) {
    if (round == max_rounds) {
      if (threadIdx.x == 0) *stuck = 1;
      return;
    }
    if (threadIdx.x == 0) remaining = 0;
    __syncthreads();
    for (unsigned i = wave; i < m; i += 16u) {
      const unsigned p = __hip_atomic_load(open_list + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const u64 left = recheck_word(bits, prev, next, p, g, lane, changed);
      if (lane == 0 && left) remaining = 1;
    }
    __syncthreads();                                         // this round's stores are visible to the next round's loads
    const int more = remaining;
    __syncthreads();
    if (!more) return;
    u64* t = prev; prev = next; next = t;
  }
}

__global__ void skel_set_int_kernel(int* p, int v) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *p = v;
}

struct SkelLayout {
  BitGeom g;
  SkelCtl* ctl;
  u64* bits;                  // the image, then the two undecided masks: planes_bytes from `bits` on hold the three padded volumes
  u64* und[2];
  size_t planes_bytes;
  unsigned *list, *open_list; // words with candidates; words still open in the single-workgroup loop
};

// false: the extents are outside what the bit layout addresses (nothing is carved)
bool skel_layout(WsCarver& c, int n0, int n1, int n2, SkelLayout* L) {
  if (n0 < 1 || n1 < 1 || n2 < 1) return false;
  const unsigned long long n = (unsigned long long)n0 * n1 * n2;
  if (n > 0x7fffffffull) return false;
  const BitGeom g = L->g = bit_geom(n0, n1, n2, 1);
  const unsigned long long padded = padded_words(g);
  if (padded > 0xffffffffull) return false;                  // the word lists hold 32-bit indices
  static_assert(sizeof(SkelCtl) <= 256, "SkelCtl outgrew its slot");
  L->ctl = c.take<SkelCtl>(1);
  const size_t planes_at = c.bytes();
  L->bits = c.take<u64>((size_t)padded);
  L->und[0] = c.take<u64>((size_t)padded);
  L->und[1] = c.take<u64>((size_t)padded);
  L->planes_bytes = c.bytes() - planes_at;
  L->list = c.take<unsigned>((size_t)g.words);
  L->open_list = c.take<unsigned>((size_t)g.words);
  return true;
}

}  // namespace

bool skeleton_ws(WsCarver& c, int n0, int n1, int n2) {
  SkelLayout L;
  return skel_layout(c, n0, n1, n2, &L);
}

size_t skeleton_workspace_bytes(int n0, int n1, int n2) {
  WsCarver c(nullptr);
  return skeleton_ws(c, n0, n1, n2) ? c.bytes() : 0;
}

int launch_skeletonize(const unsigned char* vol, int n0, int n1, int n2, unsigned char* out, int* passes_dev, void* workspace,
                       size_t ws_bytes, hipStream_t s) {
  SEUNET_CHECK(vol && out && workspace, "skeletonize: null argument");
  SEUNET_CHECK(n0 >= 1 && n1 >= 1 && n2 >= 1, "skeletonize: bad dimensions (%d, %d, %d)", n0, n1, n2);
  SkelLayout L;
  WsCarver carve(workspace);
  SEUNET_CHECK(skel_layout(carve, n0, n1, n2, &L), "skeletonize: (%d, %d, %d) exceeds 2^31-1 voxels or 2^32-1 padded 64-voxel words", n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "skeletonize: workspace too small (%zu bytes, %zu needed)", ws_bytes, carve.bytes());
  SkelCtl* ctl = L.ctl;
  u64* bits = L.bits;
  u64* const* und = L.und;
  unsigned *list = L.list, *open_list = L.open_list;
  const BitGeom g = L.g;
  const unsigned word_blocks = (unsigned)((g.words + 3) / 4);
  const unsigned round_blocks = std::min(word_blocks, 2048u);
  static const int order[6] = {4, 3, 2, 1, 5, 6};

  SEUNET_HIP(hipMemsetAsync(bits, 0, L.planes_bytes, s));    // the zero borders of the image and of both undecided masks
  pack_bits(vol, nullptr, g, bits, nullptr, s);
  int passes = 0;
  for (;;) {
    ++passes;
    SEUNET_HIP(hipMemsetAsync(ctl, 0, 256, s));
    for (int i = 0; i < 6; ++i) {
      skel_candidates_kernel<<<word_blocks, 256, 0, s>>>(bits, g, kHostTables.face[order[i] - 1], und[0], und[1], list, &ctl->count[i]);
      for (int r = 0; r < kRoundLaunches; ++r)
        skel_round_kernel<<<round_blocks, 256, 0, s>>>(bits, und[r & 1], und[(r + 1) & 1], list, &ctl->count[i], g, &ctl->changed[i]);
      skel_finish_kernel<<<1, 1024, 0, s>>>(bits, und[kRoundLaunches & 1], und[(kRoundLaunches + 1) & 1], list, open_list,
                                            &ctl->count[i], g, &ctl->changed[i], &ctl->stuck);
    }
    SEUNET_LAUNCH_CHECK();
    SkelCtl host;                                               // the one synchronisation of the pass
    SEUNET_HIP(hipMemcpyAsync(&host, ctl, sizeof(SkelCtl), hipMemcpyDeviceToHost, s));
    SEUNET_HIP(hipStreamSynchronize(s));
    SEUNET_CHECK(!host.stuck, "skeletonize: the re-check made no progress (internal error)");
    bool any = false;
    for (int i = 0; i < 6; ++i) any = any || host.changed[i] != 0;
    if (!any) break;
  }
  unpack_bits(bits, g, out, s);
  if (passes_dev) skel_set_int_kernel<<<1, 64, 0, s>>>(passes_dev, passes);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
